// Masked set-attention backward at head_dim 16 for 1 - 160 keys on the f16 matrix pipe: the training backward of the models with heads of
// 16 channels (d = 64 / 4 heads, 128 / 8, 256 / 16), which the fp32 VALU `attention_bwd_kernel<16>` served alone -- with Q, dO and the
// row statistics of all N rows of an instance in LDS (144 N bytes: no launch from N = 1131 rows).  Same inputs and outputs as that
// kernel, plus the scale word of dA (read) and of dQKV (written).  The mathematics: header of attn_bwd8.h.
//
// head_dim 16 is the native shape of v_mfma_f32_16x16x16_f16: a head's channels are exactly ONE k-step of S = Q K^T and dP = dO V^T and
// exactly the 16 M-rows of dK^T / dV^T / dQ^T -- no zero half of a tile (attn_bwd8.h), no second k-step (head_dim 32 / 64).
//   * One workgroup of 8 waves per instance, the heads in rounds of 4, TWO waves per head: they take alternate 16-row tiles and share the
//     head's K / V operands, packed (hi | lo) in LDS and staged once per round by both (alternate key tiles): KB / VB (B operands of S^T /
//     dP^T) and KA (K^T, the A operand of dQ^T), [3][NKT][64 lanes][4 words] = 30 KB per head at ten key tiles.
//   * Every product is the 3-term f16 split (hi hi + hi lo + lo hi, fp32 accumulators).  dO is scaled at the staging by the power of two
//     of max |dA| (tailbwd::grad_scale16), the scale leaves with the stores.
//   * Per (row tile, key tile): S^T and dP^T are one batch of 3 MFMA each; P and dS go from the accumulators straight into the B operand
//     of the dV^T / dK^T updates (the four accumulator registers of a lane are the k-slice of rows 4 g .. 4 g + 3); one 16 x 16 transpose
//     of dS through the wave's LDS slot feeds dQ^T.
//   * One exact softmax per row tile: the scores of all its key tiles stay in registers (4 per tile, <= 40) through maximum, exp2 and
//     sum; dP / dS exist for one key tile at a time; delta = dO . O from the attention output, out of the staging registers.
//   * dK^T / dV^T of all NKT key tiles stay in accumulators over a wave's row tiles (<= 80 registers); no atomics on floats: the first
//     wave of a pair stores its sums, the second adds its own to those rows behind a barrier.
//   * The row side is STREAMED: a wave stages Q and dO of its current 16 rows only.  Beside the fixed blocks LDS holds one byte per padded
//     token row (is the row a key), from which the visible-key count of a row follows by the row-class rule of the other kernels
//     (a remaining query sees every key, every other row the context keys).  N <= 11 104 rows at 160 keys (lds_bytes).
#pragma once
#include "tail_bwd.h"
#include "kernels.h"

namespace abw16 {

using tailbwd::H8;
using tailbwd::split4;
constexpr int HD = 16, PT = 20, HEADS = 4, WAVES = 2 * HEADS;      // staged row pitch (floats): 80-byte rows, heads per round
// LDS (floats) per wave: Q | dO rows of a tile [16][PT], the transpose slot [16][16], delta [16];  per head of a round: KB | VB | KA [3][NKT][64][4]
__host__ __device__ constexpr int wave_lds_floats() { return 2 * 16 * PT + 256 + 16; }
__host__ __device__ constexpr int head_lds_floats(int nkt) { return 3 * nkt * 256; }
// key list [16 nkt] + counters [8] | wave blocks | head blocks | one byte per padded row
__host__ __device__ inline size_t lds_bytes(int nkt, int N) {
  const int npad = (N + 15) / 16 * 16;
  return (size_t)(16 * nkt + 8) * 4 + (size_t)(WAVES * wave_lds_floats() + HEADS * head_lds_floats(nkt)) * 4 + (size_t)npad;
}
// the instantiation that serves a key count: at most three empty key tiles
__host__ __device__ constexpr int nkt_for(int max_keys) { return max_keys <= 64 ? 4 : max_keys <= 112 ? 7 : 10; }

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void mfma3(f32x4 &acc, const H8 &a, const H8 &b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.lo, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.hi, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 pack(const f32x4 &v) {      // (hi x 4 | lo x 4) of four floats: the 16 bytes tailbwd::as_h8 reads back
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const H8 s8 = split4(v);
  const u2 ph = __builtin_bit_cast(u2, s8.hi), pl = __builtin_bit_cast(u2, s8.lo);
  return (f32x4){__uint_as_float(ph[0]), __uint_as_float(ph[1]), __uint_as_float(pl[0]), __uint_as_float(pl[1])};
}

// d = 16 H; out_absmax (or null): receives the bits of max |dQKV|; dA_max_bits: bits of max |dA|
template <int NKT>
__global__ __launch_bounds__(64 * WAVES) void attention_bwd16_kernel(Geo g, int d, const float *__restrict__ QKV, const float *__restrict__ dA,
                                                                     const float *__restrict__ Aout, float *__restrict__ dQKV,
                                                                     unsigned *out_absmax, const unsigned *__restrict__ dA_max_bits) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.x;
  const int npad = (g.N + 15) / 16 * 16, n_t = g.n_td + g.n_th, H = d / HD;
  int *keyrow = reinterpret_cast<int *>(lds);            // [16 NKT] token row of a key, -1 behind the instance's last key
  int *cnt = keyrow + 16 * NKT;                           // [8] n_ck, n_ak
  float *wl = reinterpret_cast<float *>(cnt + 8) + (size_t)wave * wave_lds_floats();
  float *Qs = wl, *Gs = Qs + 16 * PT, *Ts = Gs + 16 * PT, *Dl = Ts + 256;
  const int hs = wave & (HEADS - 1), half = wave >> 2;    // head slot of the round; two waves per head: alternate row tiles
  float *KBs = reinterpret_cast<float *>(cnt + 8) + (size_t)WAVES * wave_lds_floats() + (size_t)hs * head_lds_floats(NKT);
  float *VBs = KBs + NKT * 256, *KAs = VBs + NKT * 256;
  unsigned char *iskey = reinterpret_cast<unsigned char *>(reinterpret_cast<float *>(cnt + 8) + (size_t)WAVES * wave_lds_floats() +
                                                           (size_t)HEADS * head_lds_floats(NKT));      // [npad]
  const long ep = (long)b * g.N;
  // ---- key list (context rows in slot order, then the visible targets), by wave 0 (attn_bwd8.h) -------------------------------------
  if (wave == 0) {
    int n = 0;
    for (int c0 = 0; c0 < npad; c0 += 64) {
      const int row = c0 + lane;
      const bool key = row < g.P && is_ctx(g, b, row);
      const unsigned long long bal = __ballot(key);
      const int k = n + __popcll(bal & ((1ull << lane) - 1ull));
      if (row < npad) iskey[row] = (key && k < 16 * NKT) ? 1 : 0;
      if (key && k < 16 * NKT) keyrow[k] = row;
      n += __popcll(bal);
    }
    n = min(n, 16 * NKT);
    const int n_ck = n;
    for (int c0 = 0; c0 < n_t; c0 += 64) {
      const int j = c0 + lane;
      const bool key = j < n_t && (!g.tmask || g.tmask[j]);
      const unsigned long long bal = __ballot(key);
      const int k = n + __popcll(bal & ((1ull << lane) - 1ull));
      if (key && k < 16 * NKT) { keyrow[k] = g.P + j; iskey[g.P + j] = 1; }
      n += __popcll(bal);
    }
    n = min(n, 16 * NKT);
    if (lane == 0) { cnt[0] = n_ck; cnt[1] = n; }
    for (int k = n + lane; k < 16 * NKT; k += 64) keyrow[k] = -1;
  }
  __syncthreads();
  const int n_ck = __builtin_amdgcn_readfirstlane(cnt[0]), n_ak = __builtin_amdgcn_readfirstlane(cnt[1]);
  const int nkt_all = (n_ak + 15) >> 4, nkt_ctx = (n_ck + 15) >> 4;
  float ginv;
  const float gs = tailbwd::grad_scale16(*dA_max_bits, ginv);
  const float scale = rsqrtf((float)HD) * 1.44269504088896340736f;      // scores in base-2 units; dQ / dK get 1 / sqrt(hd) = scale * ln 2 at the end
  const float oscale = rsqrtf((float)HD) * ginv, kscale = 0.69314718055994530942f * ginv;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  unsigned omax = 0;
  auto track = [&](const f32x4 &v) {
    omax = max(max(omax, __float_as_uint(v[0]) & 0x7fffffffu), max(__float_as_uint(v[1]) & 0x7fffffffu, max(__float_as_uint(v[2]) & 0x7fffffffu, __float_as_uint(v[3]) & 0x7fffffffu)));
  };
  for (int h0 = 0; h0 < H; h0 += HEADS) {
    // (H no multiple of 4: the pairs past the last head repeat it in their own LDS blocks and store nothing -- the barriers stay whole)
    const bool live = h0 + hs < H;
    const int h = min(h0 + hs, H - 1);
    const int qc = h * HD, kc = d + h * HD, vc = 2 * d + h * HD;
    // ---- K / V of the head's key rows, once per round, the key tiles alternating between the pair: KB / VB [kt]: B operands of S / dP
    // (n = key fr, k = channels 4 g .. 4 g + 3);  KA [kt]: A operand of dQ^T (m = channel fr, k = keys 4 g .. 4 g + 3 of the tile)
    f32x4 dKT[NKT], dVT[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      dKT[kt] = z4; dVT[kt] = z4;
      if (kt < nkt_all && (kt & 1) == half) {
        const int kr = keyrow[16 * kt + fr];
        f32x4 kv = z4, vv = z4;
        if (kr >= 0) {
          const float *kp = QKV + (ep + kr) * 3 * d;
          kv = *reinterpret_cast<const f32x4 *>(kp + kc + 4 * fg);
          vv = *reinterpret_cast<const f32x4 *>(kp + vc + 4 * fg);
        }
        *reinterpret_cast<f32x4 *>(KBs + (kt * 64 + lane) * 4) = pack(kv);
        *reinterpret_cast<f32x4 *>(VBs + (kt * 64 + lane) * 4) = pack(vv);
        f32x4 ka = z4;
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) {
          const int kr2 = keyrow[16 * kt + 4 * fg + sp];
          if (kr2 >= 0) ka[sp] = QKV[(ep + kr2) * 3 * d + kc + fr];
        }
        *reinterpret_cast<f32x4 *>(KAs + (kt * 64 + lane) * 4) = pack(ka);
      }
    }
    __syncthreads();
    // ---- the wave's row tiles ---------------------------------------------------------------------------------------------------------
    for (int r0 = 16 * half; r0 < npad; r0 += 32) {
      // stage Q (base-2 scale) and dO (scaled by gs) of the 16 rows: four lanes per row of 16 floats; delta_row = gs dO . O over the four
      {
        const int rr = lane >> 2, c4 = 4 * (lane & 3), row = r0 + rr;
        f32x4 q = z4, go = z4, oo = z4;
        if (row < g.N) {
          q = *reinterpret_cast<const f32x4 *>(QKV + (ep + row) * 3 * d + qc + c4);
          go = *reinterpret_cast<const f32x4 *>(dA + (ep + row) * d + qc + c4);
          oo = *reinterpret_cast<const f32x4 *>(Aout + (ep + row) * d + qc + c4);
        }
        go = go * gs;
        *reinterpret_cast<f32x4 *>(Qs + rr * PT + c4) = q * scale;
        *reinterpret_cast<f32x4 *>(Gs + rr * PT + c4) = go;
        float dl = fmaf(go[0], oo[0], fmaf(go[1], oo[1], fmaf(go[2], oo[2], go[3] * oo[3])));
        dl += __shfl_xor(dl, 1, 64);
        dl += __shfl_xor(dl, 2, 64);
        if ((lane & 3) == 0) Dl[rr] = dl;
      }
      // (the wave's own LDS traffic is ordered: no barrier)  QA / GA: A of S / dP (m = row fr, k = channels 4 g ..);  QTA / GTA: A of
      // dK^T / dV^T (m = channel fr, k = rows 4 g ..)
      f32x4 qta, gta;
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) { qta[sp] = Qs[(4 * fg + sp) * PT + fr]; gta[sp] = Gs[(4 * fg + sp) * PT + fr]; }
      const H8 QA = split4(*reinterpret_cast<const f32x4 *>(Qs + fr * PT + 4 * fg)), GA = split4(*reinterpret_cast<const f32x4 *>(Gs + fr * PT + 4 * fg));
      const H8 QTA = split4(qta), GTA = split4(gta);
      const f32x4 dl4 = *reinterpret_cast<const f32x4 *>(Dl + 4 * fg);
      // keys visible to rows 4 g + r: a remaining query (a point row that is no key) sees all of them, every other row the context keys
      const unsigned kb4 = *reinterpret_cast<const unsigned *>(iskey + r0 + 4 * fg);
      int nvr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * fg + r;
        const bool isq = row < g.P && !((kb4 >> (8 * r)) & 1u);
        nvr[r] = row < g.N ? (isq ? n_ak : n_ck) : 0;
      }
      const int nkt = r0 < g.P ? nkt_all : nkt_ctx;          // (wave-uniform) a tile without point rows sees the context keys only
      // sweep 1: the scores of every key tile (kept: 4 registers per tile), their maximum per row; then e = 2^(s - max) in place and the sum
      f32x4 S[NKT];
      f32x4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sum = z4;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt < nkt) {
          S[kt] = z4;
          mfma3(S[kt], QA, tailbwd::as_h8(*reinterpret_cast<const f32x4 *>(KBs + (kt * 64 + lane) * 4)));
          const int key = 16 * kt + fr;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            S[kt][r] = key < nvr[r] ? S[kt][r] : -INFINITY;
            mx[r] = fmaxf(mx[r], S[kt][r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[r] = group16_max(mx[r]);
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt < nkt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = mx[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(S[kt][r] - mx[r]);      // (a masked score: 2^-inf = 0; a row without keys: 0)
            S[kt][r] = e;
            sum[r] += e;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float l = group16_sum(sum[r]); sum[r] = l > 0.f ? 1.f / l : 0.f; }
      // sweep 2: P, dS;  dV^T += dO^T P,  dK^T += Q^T dS;  dQ^T += K^T dS^T through the transpose slot
      f32x4 dQT = z4;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt < nkt) {
          f32x4 dP = z4;
          mfma3(dP, GA, tailbwd::as_h8(*reinterpret_cast<const f32x4 *>(VBs + (kt * 64 + lane) * 4)));
          f32x4 P, dS;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            P[r] = S[kt][r] * sum[r];
            dS[r] = P[r] * (dP[r] - dl4[r]);
          }
          const H8 PS = split4(P), dSS = split4(dS);
          mfma3(dVT[kt], GTA, PS);
          mfma3(dKT[kt], QTA, dSS);
          // transpose dS: write [row 4 g + r][key fr], read [row fr][keys 4 g .. 4 g + 3]
#pragma unroll
          for (int r = 0; r < 4; ++r) Ts[(4 * fg + r) * 16 + fr] = dS[r];
          const H8 dST = split4(*reinterpret_cast<const f32x4 *>(Ts + fr * 16 + 4 * fg));
          mfma3(dQT, tailbwd::as_h8(*reinterpret_cast<const f32x4 *>(KAs + (kt * 64 + lane) * 4)), dST);
        }
      }
      // dQ of the tile (channels 4 g + r of row fr), zeros for the K / V gradient slices of the rows that are not keys
      const int row = r0 + fr;
      if (row < g.N && live) {
        float *out = dQKV + (ep + row) * 3 * d;
        const f32x4 o = dQT * oscale;
        track(o);
        *reinterpret_cast<f32x4 *>(out + qc + 4 * fg) = o;
        if (!iskey[row]) {
          *reinterpret_cast<f32x4 *>(out + kc + 4 * fg) = z4;
          *reinterpret_cast<f32x4 *>(out + vc + 4 * fg) = z4;
        }
      }
    }
    // ---- dK / dV of the head's key rows (Q was staged with the base-2 scale: dK takes ln 2): the first wave of a pair stores its sums,
    // the second adds its own behind a barrier (same CU: the rows come back from its L1 / L2) and sees the final values for the scale
    // word.  The last barrier also frees the head blocks for the next round. -----------------------------------------------------------
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == half && live) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          if (kt < nkt_all) {
            const int kr = keyrow[16 * kt + fr];
            if (kr >= 0) {
              float *out = dQKV + (ep + kr) * 3 * d;
              f32x4 dk = dKT[kt] * kscale, dv = dVT[kt] * ginv;
              if (pass == 1) {
                dk += *reinterpret_cast<const f32x4 *>(out + kc + 4 * fg); dv += *reinterpret_cast<const f32x4 *>(out + vc + 4 * fg);
                track(dk); track(dv);
              }
              *reinterpret_cast<f32x4 *>(out + kc + 4 * fg) = dk;
              *reinterpret_cast<f32x4 *>(out + vc + 4 * fg) = dv;
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (out_absmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omax = max(omax, (unsigned)__shfl_xor((int)omax, o, 64));
    if (lane == 0 && omax) atomicMax(out_absmax, omax);
  }
}

}  // namespace abw16
