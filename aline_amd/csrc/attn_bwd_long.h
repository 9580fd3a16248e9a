// Masked set-attention backward at head_dim 32 for 4 - 10 key tiles (49 - 160 keys) on the f16 matrix pipe: the kernel of attn_bwd_wide.h
// (same inputs, same outputs, same 3-term split and power-of-two scaling as abww::attention_bwd_wide16_kernel) with a head's key tiles
// split over a group of waves.  One wave per head cannot hold more than three key tiles (dK^T / dV^T accumulators and both K / V operand
// layouts of every tile: <32, 4> spills 64 registers), and the fp32 VALU kernel that served these shapes keeps K, V, dK, dV of the
// instance and Q, dO of every row in LDS (max_keys * 516 + N * 272 bytes: no launch beyond N = 295 rows at 160 keys).
//
// One workgroup of 8 waves per instance.  A head is worked by a group of G waves, 8 / G heads at once, the heads in rounds.  Wave j of a
// group owns the key tiles j, G + j, 2 G + j (at most TPW of them; a tile past the instance's last key is skipped):
//   * K / V of its tiles are loaded once per head in both operand layouts (the B operands of S / dP into registers, K^T for dQ^T into the
//     wave's LDS, already split), dK^T / dV^T of its tiles stay in registers over all row tiles and leave with plain stores: no second
//     wave adds to them.
//   * the Q / dO rows of a row tile are staged in LDS once per group (the first 128 threads of the group: 8 lanes per row, float4), delta
//     comes out of the staging registers (dO . O over the 8 lanes of a row): O never enters LDS.
//   * softmax statistics: a wave writes (max, sum exp(s - max)) of each row over its own tiles; after the barrier every wave of the group
//     combines the G pairs in the order j = 0 .. G - 1, so all of them use the same (max, 1 / sum) whatever the timing.
//   * dQ^T of a row tile is the sum of the group's partials: each wave writes its partial to LDS, after the next barrier ONE wave of the
//     group (in turn: row tile mod G) adds them in the order j = 0 .. G - 1, scales and stores.  No atomics on floats.
// Two workgroup barriers per row tile (every wave runs the same trip counts):
//   A: staged rows + dQ partials of the previous tile visible | operands to registers, S, dP, local statistics
//   B: statistics visible, staged rows consumed               | stage the next tile, P, dS, dV^T, dK^T, dQ^T partial
// LDS: the key list and two ints per padded row, 8 / G group blocks (2 row images, delta, statistics, dQ exchange), a transpose slot and K^T per wave.
#pragma once
#include "common.h"
#include "kernels.h"
#include "tail_bwd.h"
#include "attn_bwd_wide.h"

namespace abwl {

constexpr int WAVES = 8, HD = 32, PT = HD + 4, NCT = HD / 16, NG = HD / 16;
// floats of a group block: Q | dO rows [16][PT], delta [16], statistics [G][16][2], dQ^T partials [G][NCT][64 lanes][4]
__host__ __device__ constexpr int group_lds_floats(int G) { return 2 * 16 * PT + 16 + G * 32 + G * NCT * 256; }
// floats of a wave: the transpose slot [16][16], K^T of its key tiles as split A operands [TPW][NCT][64 lanes][hi hi lo lo]
__host__ __device__ constexpr int wave_lds_floats(int tpw) { return 256 + tpw * NCT * 256; }
__host__ __device__ inline size_t lds_bytes(int tpw, int G, int N) {
  const int npad = (N + 15) / 16 * 16;
  return (size_t)(16 * tpw * G + 2 * npad + 8) * 4 + (size_t)(WAVES / G) * group_lds_floats(G) * 4 + (size_t)WAVES * wave_lds_floats(tpw) * 4;
}

template <int TPW, int G>
__global__ __launch_bounds__(64 * WAVES) void attention_bwd_long_kernel(Geo g, int d, const float *__restrict__ QKV, const float *__restrict__ dA,
                                                                        const float *__restrict__ Aout, float *__restrict__ dQKV,
                                                                        unsigned *out_absmax, const unsigned *__restrict__ dA_max_bits) {
  using tailbwd::H8;
  using tailbwd::split4;
  constexpr int NKT = TPW * G, HPR = WAVES / G;      // key tiles the group holds, heads per round
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gi = wave / G, j = wave % G;              // head group, place in the group
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.x;
  const int npad = (g.N + 15) / 16 * 16, n_t = g.n_td + g.n_th, H = d / HD;
  int *keyrow = reinterpret_cast<int *>(lds);            // [16 NKT]
  int *nvis = keyrow + 16 * NKT;                          // [npad] keys visible to a row (0 for the padding rows)
  int *kidx = nvis + npad;                                // [npad] position of a row in the key list, or -1
  int *cnt = kidx + npad;                                 // [8] n_ck, n_ak
  float *gl = reinterpret_cast<float *>(cnt + 8) + (size_t)gi * group_lds_floats(G);
  float *Qs = gl, *Gs = Qs + 16 * PT, *Dl = Gs + 16 * PT, *St = Dl + 16, *Xq = St + G * 32;
  float *Ts = reinterpret_cast<float *>(cnt + 8) + (size_t)HPR * group_lds_floats(G) + (size_t)wave * wave_lds_floats(TPW), *Kt = Ts + 256;
  const long ep = (long)b * g.N;
  // ---- key list (context rows in slot order, then the visible targets) and the per-row visibility, by wave 0 (attn_bwd_wide.h) ------
  if (wave == 0) {
    int n = 0;
    for (int c0 = 0; c0 < npad; c0 += 64) {
      const int row = c0 + lane;
      const bool key = row < g.P && is_ctx(g, b, row);
      const unsigned long long bal = __ballot(key);
      const int k = n + __popcll(bal & ((1ull << lane) - 1ull));
      if (row < npad) kidx[row] = (key && k < 16 * NKT) ? k : -1;
      if (key && k < 16 * NKT) keyrow[k] = row;
      n += __popcll(bal);
    }
    n = min(n, 16 * NKT);
    const int n_ck = n;
    for (int c0 = 0; c0 < n_t; c0 += 64) {
      const int jt = c0 + lane;
      const bool key = jt < n_t && (!g.tmask || g.tmask[jt]);
      const unsigned long long bal = __ballot(key);
      const int k = n + __popcll(bal & ((1ull << lane) - 1ull));
      if (key && k < 16 * NKT) { keyrow[k] = g.P + jt; kidx[g.P + jt] = k; }
      n += __popcll(bal);
    }
    n = min(n, 16 * NKT);
    if (lane == 0) { cnt[0] = n_ck; cnt[1] = n; }
    for (int k = n + lane; k < 16 * NKT; k += 64) keyrow[k] = -1;
  }
  __syncthreads();
  const int n_ck = cnt[0], n_ak = __builtin_amdgcn_readfirstlane(cnt[1]);
  for (int row = tid; row < npad; row += blockDim.x) {
    const bool isq = row < g.P && kidx[row] < 0;          // (a point row that is not a context key is a remaining query)
    nvis[row] = row < g.N ? (isq ? n_ak : n_ck) : 0;
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  float ginv;
  const float gs = tailbwd::grad_scale16(*dA_max_bits, ginv);
  auto mfma3 = [](f32x4 &acc, const H8 &a, const H8 &bb) {
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.lo, bb.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, bb.lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, bb.hi, acc, 0, 0, 0);
  };
  unsigned omax = 0;
  auto track = [&](const f32x4 &v) {
    omax = max(max(omax, __float_as_uint(v[0]) & 0x7fffffffu), max(__float_as_uint(v[1]) & 0x7fffffffu, max(__float_as_uint(v[2]) & 0x7fffffffu, __float_as_uint(v[3]) & 0x7fffffffu)));
  };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const int ntile = npad / 16;
  for (int h0 = 0; h0 < H; h0 += HPR) {
    // (H no multiple of 8 / G: the groups past the last head repeat it in their own LDS block and store nothing -- the barriers stay whole)
    const bool live = h0 + gi < H;
    const int h = min(h0 + gi, H - 1);
    const int qc = h * HD, kc = d + h * HD, vc = 2 * d + h * HD;
    // stage Q (scaled by 1 / sqrt(hd)) and dO (scaled by gs) of the 16 rows from r0, delta_row = gs dO . O
    auto stage = [&](int r0) {
      if (j < 2) {
        const int s = 64 * j + lane, rr = s >> 3, c4 = 4 * (s & 7), row = r0 + rr;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), go = q, oo = q;
        if (row < g.N) {
          q = *reinterpret_cast<const float4 *>(QKV + (ep + row) * 3 * d + qc + c4);
          go = *reinterpret_cast<const float4 *>(dA + (ep + row) * d + qc + c4);
          oo = *reinterpret_cast<const float4 *>(Aout + (ep + row) * d + qc + c4);
        }
        q.x *= scale; q.y *= scale; q.z *= scale; q.w *= scale;
        go.x *= gs; go.y *= gs; go.z *= gs; go.w *= gs;
        *reinterpret_cast<float4 *>(Qs + rr * PT + c4) = q;
        *reinterpret_cast<float4 *>(Gs + rr * PT + c4) = go;
        float dl = fmaf(go.x, oo.x, fmaf(go.y, oo.y, fmaf(go.z, oo.z, go.w * oo.w)));
        dl += __shfl_xor(dl, 1, 64);
        dl += __shfl_xor(dl, 2, 64);
        dl += __shfl_xor(dl, 4, 64);
        if ((s & 7) == 0) Dl[rr] = dl;
      }
    };
    // dQ of the row tile from r0: the group's partials in the order of the waves, by the calling wave alone
    auto store_dq = [&](int r0) {
      f32x4 v[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        v[ct] = *reinterpret_cast<const f32x4 *>(Xq + (ct * 64 + lane) * 4);
#pragma unroll
        for (int jj = 1; jj < G; ++jj) v[ct] += *reinterpret_cast<const f32x4 *>(Xq + ((jj * NCT + ct) * 64 + lane) * 4);
      }
      const int row = r0 + fr;
      if (row < g.N && live) {      // channels 16 ct + 4 g + r of row fr; zeros for the K / V gradient slices of the rows that are not keys
        float *out = dQKV + (ep + row) * 3 * d;
        const bool notkey = kidx[row] < 0;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const f32x4 o = v[ct] * (scale * ginv);
          track(o);
          *reinterpret_cast<f32x4 *>(out + qc + 16 * ct + 4 * fg) = o;
          if (notkey) {
            *reinterpret_cast<f32x4 *>(out + kc + 16 * ct + 4 * fg) = z4;
            *reinterpret_cast<f32x4 *>(out + vc + 16 * ct + 4 * fg) = z4;
          }
        }
      }
    };
    // ---- K / V of the wave's key tiles, once, in both operand layouts (attn_bwd_wide.h) -------------------------------------------
    // (the A operand of dQ^T, K^T with the keys 4 g .. 4 g + 3 of the tile on a lane, waits in the wave's LDS: 8 registers per tile less)
    H8 KB[TPW][NG], VB[TPW][NG];
    f32x4 dKT[TPW][NCT], dVT[TPW][NCT];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int kt = t * G + j;
      const int kr = keyrow[16 * kt + fr];
      const float *kp = QKV + (ep + max(kr, 0)) * 3 * d;
#pragma unroll
      for (int kg = 0; kg < NG; ++kg) {
        const f32x4 kv = kr >= 0 ? *reinterpret_cast<const f32x4 *>(kp + kc + 16 * kg + 4 * fg) : z4;
        const f32x4 vv = kr >= 0 ? *reinterpret_cast<const f32x4 *>(kp + vc + 16 * kg + 4 * fg) : z4;
        KB[t][kg] = split4(kv); VB[t][kg] = split4(vv);
      }
      f32x4 ka[NCT];
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) {
        const int kr2 = keyrow[16 * kt + 4 * fg + sp];
        const float *kp2 = QKV + (ep + max(kr2, 0)) * 3 * d + kc;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) ka[ct][sp] = kr2 >= 0 ? kp2[16 * ct + fr] : 0.f;
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        const H8 ks = split4(ka[ct]);
        const u2 hi = __builtin_bit_cast(u2, ks.hi), lo = __builtin_bit_cast(u2, ks.lo);
        *reinterpret_cast<f32x4 *>(Kt + ((t * NCT + ct) * 64 + lane) * 4) = (f32x4){__uint_as_float(hi[0]), __uint_as_float(hi[1]), __uint_as_float(lo[0]), __uint_as_float(lo[1])};
        dKT[t][ct] = z4; dVT[t][ct] = z4;
      }
    }
    stage(0);
    // ---- row tiles -----------------------------------------------------------------------------------------------------------------
    for (int rt = 0; rt < ntile; ++rt) {
      const int r0 = 16 * rt;
      __syncthreads();      // A
      if (rt > 0 && (rt - 1) % G == j) store_dq(r0 - 16);
      H8 QA[NG], GA[NG], QTA[NCT], GTA[NCT];
#pragma unroll
      for (int kg = 0; kg < NG; ++kg) {
        QA[kg] = split4(*reinterpret_cast<const f32x4 *>(Qs + fr * PT + 16 * kg + 4 * fg));
        GA[kg] = split4(*reinterpret_cast<const f32x4 *>(Gs + fr * PT + 16 * kg + 4 * fg));
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        f32x4 qt, gt;
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) { qt[sp] = Qs[(4 * fg + sp) * PT + 16 * ct + fr]; gt[sp] = Gs[(4 * fg + sp) * PT + 16 * ct + fr]; }
        QTA[ct] = split4(qt); GTA[ct] = split4(gt);
      }
      const int4 nv = *reinterpret_cast<const int4 *>(nvis + r0 + 4 * fg);
      const f32x4 dl4 = *reinterpret_cast<const f32x4 *>(Dl + 4 * fg);
      // S and dP of the wave's key tiles; the statistics of rows 4 g + r over them
      f32x4 S[TPW], dP[TPW];
      f32x4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int kt = t * G + j, key = 16 * kt + fr;
        S[t] = z4; dP[t] = z4;
        if (16 * kt < n_ak) {
#pragma unroll
          for (int kg = 0; kg < NG; ++kg) { mfma3(S[t], QA[kg], KB[t][kg]); mfma3(dP[t], GA[kg], VB[t][kg]); }
        }
        S[t][0] = key < nv.x ? S[t][0] : -INFINITY; S[t][1] = key < nv.y ? S[t][1] : -INFINITY;
        S[t][2] = key < nv.z ? S[t][2] : -INFINITY; S[t][3] = key < nv.w ? S[t][3] : -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], S[t][r]);
      }
      f32x4 sum = z4;
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[r] = abww::group16_max(mx[r]);
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = mx[r] == -INFINITY ? 0.f : __expf(S[t][r] - mx[r]);      // (rows that see none of the wave's keys: all zero)
          S[t][r] = e;
          sum[r] += e;
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] = abww::group16_sum(sum[r]);
      if (fr == 0) {
        *reinterpret_cast<f32x4 *>(St + j * 32 + 8 * fg) = (f32x4){mx[0], sum[0], mx[1], sum[1]};
        *reinterpret_cast<f32x4 *>(St + j * 32 + 8 * fg + 4) = (f32x4){mx[2], sum[2], mx[3], sum[3]};
      }
      __syncthreads();      // B
      if (rt + 1 < ntile) stage(r0 + 16);
      // the row's statistics over the group: M = max_j m_j, L = sum_j l_j exp(m_j - M), j in order; this wave's factor exp(m - M) / L
      f32x4 fac;
      {
        float m[G][4], l[G][4];
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
          const f32x4 a = *reinterpret_cast<const f32x4 *>(St + jj * 32 + 8 * fg), c = *reinterpret_cast<const f32x4 *>(St + jj * 32 + 8 * fg + 4);
          m[jj][0] = a[0]; l[jj][0] = a[1]; m[jj][1] = a[2]; l[jj][1] = a[3];
          m[jj][2] = c[0]; l[jj][2] = c[1]; m[jj][3] = c[2]; l[jj][3] = c[3];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float M = m[0][r];
#pragma unroll
          for (int jj = 1; jj < G; ++jj) M = fmaxf(M, m[jj][r]);
          float L = 0.f;
#pragma unroll
          for (int jj = 0; jj < G; ++jj) L += m[jj][r] == -INFINITY ? 0.f : l[jj][r] * __expf(m[jj][r] - M);
          fac[r] = (mx[r] == -INFINITY || !(L > 0.f)) ? 0.f : __expf(mx[r] - M) / L;
        }
      }
      // P, dS;  dV^T += dO^T P,  dK^T += Q^T dS;  dQ^T partial += K^T dS^T through the transpose slot
      f32x4 dQT[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) dQT[ct] = z4;
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        if (16 * (t * G + j) < n_ak) {
          f32x4 P, dS;
#pragma unroll
          for (int r = 0; r < 4; ++r) { P[r] = S[t][r] * fac[r]; dS[r] = P[r] * (dP[t][r] - dl4[r]); }
          const H8 PS = split4(P), dSS = split4(dS);
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) { mfma3(dVT[t][ct], GTA[ct], PS); mfma3(dKT[t][ct], QTA[ct], dSS); }
          // transpose dS: write [row 4 g + r][key fr], read [row fr][keys 4 g .. 4 g + 3] (the wave's own slot: no barrier)
#pragma unroll
          for (int r = 0; r < 4; ++r) Ts[(4 * fg + r) * 16 + fr] = dS[r];
          const H8 dST = split4(*reinterpret_cast<const f32x4 *>(Ts + fr * 16 + 4 * fg));
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) mfma3(dQT[ct], tailbwd::as_h8(*reinterpret_cast<const f32x4 *>(Kt + ((t * NCT + ct) * 64 + lane) * 4)), dST);
        }
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) *reinterpret_cast<f32x4 *>(Xq + ((j * NCT + ct) * 64 + lane) * 4) = dQT[ct];
    }
    __syncthreads();
    if ((ntile - 1) % G == j) store_dq(16 * (ntile - 1));
    // ---- dK / dV of the wave's key rows (Q was staged scaled: dK carries the 1 / sqrt(hd)) -------------------------------------------
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int kr = keyrow[16 * (t * G + j) + fr];
      if (kr >= 0 && live) {
        float *out = dQKV + (ep + kr) * 3 * d;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const f32x4 dkv = dKT[t][ct] * ginv, dvv = dVT[t][ct] * ginv;
          track(dkv); track(dvv);
          *reinterpret_cast<f32x4 *>(out + kc + 16 * ct + 4 * fg) = dkv;
          *reinterpret_cast<f32x4 *>(out + vc + 16 * ct + 4 * fg) = dvv;
        }
      }
    }
  }
  if (out_absmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omax = max(omax, (unsigned)__shfl_xor((int)omax, o, 64));
    if (lane == 0 && omax) atomicMax(out_absmax, omax);
  }
}

}  // namespace abwl
