// Masked set-attention backward at head_dim 64 for 4 - 10 key tiles (49 - 160 keys) on the f16 matrix pipe: inputs, outputs, 3-term split,
// power-of-two scaling, key list and guarantees of abwl::attention_bwd_long_kernel (attn_bwd_long.h: a head's key tiles over a group of
// waves, one statistics exchange and one dQ^T exchange per row tile, no float atomics), with a tile program of its own.  At head_dim 64 a
// key tile costs 32 registers of K / V B operands and 32 of dK^T / dV^T accumulators, and the Q, dO, Q^T, dO^T operands of a row tile
// would be 64 more: abwl's program (operands of the row tile in registers, three tiles per wave) does not fit 256 registers.  Here:
//   * at most TWO key tiles per wave (128 registers of operands and accumulators).  Groups of 4 waves, two heads per round, for 4 - 8
//     tiles; one group of 8 waves, one head per round, for 9 - 10 tiles (waves 0 and 1 own two tiles, the others one).
//   * the Q / dO operands are NOT held: the group stages a row tile once, ALREADY SPLIT, as one word (hi half | lo half << 16) per element,
//     in two images -- row-major [16][PT] (A operands of S / dP) and transposed [64][PTT] (A operands of dK^T / dV^T) -- and every wave
//     streams them per 16-channel k-step: one ds_read_b128 and four half-word permutes per operand instead of a split (4 cvt + 4 cvt back
//     + 4 sub + 4 cvt) in each of the G waves, 8 live registers instead of 64.  All 256 threads of 4 waves stage (16 lanes per row, float4;
//     delta = dO . O over the 16 lanes of a row: O never enters LDS).
//   * both images are single-buffered without a third barrier.  The row-major image is read between barriers A and B only, the transposed
//     one between B and the next A only: the staging thread loads the next tile after B, writes its row-major words at once and keeps the
//     same 8 words in registers until it has passed the next A, where they go to the transposed image.
//   * K^T of the wave's tiles (A operand of dQ^T) waits in the wave's own LDS, split once per head (as abwl: no second wave reads it).
// Two workgroup barriers per row tile, the same trip counts in every wave:
//   A: row-major image, delta, dQ partials of the previous tile visible | transposed image, S, dP, local statistics
//   B: statistics and transposed image visible, row-major image consumed | row-major image of the next tile, P, dS, dV^T, dK^T, dQ^T partial
// Registers at two waves per SIMD (kernel_resources.txt): <1, 4> 198, no scratch.  <2, 4> and <2, 8> sit at 256 and miss the target of no
// scratch by 34 and 38 registers (136 / 152 bytes per lane): address words of the dQ store and of the head prologue, about 8 reloads and
// one store per row tile beside its 120 MFMAs; none of the operands or accumulators.
#pragma once
#include "common.h"
#include "kernels.h"
#include "tail_bwd.h"
#include "attn_bwd_wide.h"

namespace abwl64 {

constexpr int WAVES = 8, HD = 64, PT = HD + 4, PTT = 20, NCT = HD / 16, NG = HD / 16;
// floats of a group block: Q | dO row-major [16][PT], Q^T | dO^T [HD][PTT], delta [16], statistics [G][16][2], dQ^T partials [G][NCT][64 lanes][4]
__host__ __device__ constexpr int group_lds_floats(int G) { return 2 * 16 * PT + 2 * HD * PTT + 16 + G * 32 + G * NCT * 256; }
// floats of a wave: the transpose slot [16][16], K^T of its key tiles as split A operands [TPW][NCT][64 lanes][hi hi lo lo]
__host__ __device__ constexpr int wave_lds_floats(int tpw) { return 256 + tpw * NCT * 256; }
// <1, 4>: 113 056 bytes, <2, 4>: 146 080, <2, 8>: 127 584, each + 8 bytes per padded row (N = 512 at 160 keys: 131 680; <2, 4> holds 2 208 rows)
__host__ __device__ inline size_t lds_bytes(int tpw, int G, int N) {
  const int npad = (N + 15) / 16 * 16;
  return (size_t)(16 * tpw * G + 2 * npad + 8) * 4 + (size_t)(WAVES / G) * group_lds_floats(G) * 4 + (size_t)WAVES * wave_lds_floats(tpw) * 4;
}

typedef unsigned u2 __attribute__((ext_vector_type(2)));
// two words of two halves each: (x.lo | y.lo << 16, x.hi | y.hi << 16) -- a 2 x 2 transpose of halves, its own inverse
__device__ __forceinline__ u2 zip16(unsigned x, unsigned y) { return (u2){(x & 0xffffu) | (y << 16), (x >> 16) | (y & 0xffff0000u)}; }
// the staged form of four values: per element one word, hi half | lo half << 16
__device__ __forceinline__ f32x4 pack4(const f32x4 &v) {
  const tailbwd::H8 s = tailbwd::split4(v);
  const u2 hi = __builtin_bit_cast(u2, s.hi), lo = __builtin_bit_cast(u2, s.lo);
  const u2 a = zip16(hi[0], lo[0]), b = zip16(hi[1], lo[1]);
  return (f32x4){__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(b[0]), __uint_as_float(b[1])};
}
// ... and back to the operand pair of the matrix pipe
__device__ __forceinline__ tailbwd::H8 unpack4(const f32x4 &w) {
  const u2 a = zip16(__float_as_uint(w[0]), __float_as_uint(w[1])), b = zip16(__float_as_uint(w[2]), __float_as_uint(w[3]));
  const u2 hi = {a[0], b[0]}, lo = {a[1], b[1]};
  tailbwd::H8 o;
  o.hi = __builtin_bit_cast(tailbwd::h4, hi);
  o.lo = __builtin_bit_cast(tailbwd::h4, lo);
  return o;
}

template <int TPW, int G>
__global__ __launch_bounds__(64 * WAVES) void attention_bwd_long64_kernel(Geo g, int d, const float *__restrict__ QKV, const float *__restrict__ dA,
                                                                          const float *__restrict__ Aout, float *__restrict__ dQKV,
                                                                          unsigned *out_absmax, const unsigned *__restrict__ dA_max_bits) {
  using tailbwd::H8;
  using tailbwd::split4;
  static_assert(TPW >= 1 && TPW <= 2 && (G == 4 || G == 8), "two tiles per wave at most; 4 waves stage a row tile");
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
  float *Qr = gl, *Gr = Qr + 16 * PT, *Qt = Gr + 16 * PT, *Gt = Qt + HD * PTT, *Dl = Gt + HD * PTT, *St = Dl + 16, *Xq = St + G * 32;
  float *Ts = reinterpret_cast<float *>(cnt + 8) + (size_t)HPR * group_lds_floats(G) + (size_t)wave * wave_lds_floats(TPW), *Kt = Ts + 256;
  const long ep = (long)b * g.N;
  // ---- key list (context rows in slot order, then the visible targets) and the per-row visibility, by wave 0 (attn_bwd_long.h) ------
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
  // the staging thread's place: row rr of the tile, channels c4 .. c4 + 3 (waves 0 - 3 of the group)
  const int ss = 64 * (j & 3) + lane, srr = ss >> 4, sc4 = 4 * (ss & 15);
  for (int h0 = 0; h0 < H; h0 += HPR) {
    // (H no multiple of 8 / G: the groups past the last head repeat it in their own LDS block and store nothing -- the barriers stay whole)
    const bool live = h0 + gi < H;
    const int h = min(h0 + gi, H - 1);
    const int qc = h * HD, kc = d + h * HD, vc = 2 * d + h * HD;
    // Q (scaled by 1 / sqrt(hd)) and dO (scaled by gs) of the 16 rows from r0, split and packed: the row-major image and delta_row = gs dO . O
    // now, the same words (tq, tg) to the transposed image after the next barrier A
    f32x4 tq = z4, tg = z4, sq = z4, sg = z4, so = z4;
    auto load_rows = [&](int r0) {      // (issued right after barrier B: the latency passes behind the products)
      if (j < 4) {
        const int row = r0 + srr;
        sq = z4; sg = z4; so = z4;
        if (row < g.N) {
          sq = *reinterpret_cast<const f32x4 *>(QKV + (ep + row) * 3 * d + qc + sc4);
          sg = *reinterpret_cast<const f32x4 *>(dA + (ep + row) * d + qc + sc4);
          so = *reinterpret_cast<const f32x4 *>(Aout + (ep + row) * d + qc + sc4);
        }
      }
    };
    auto put_rows = [&]() {
      if (j < 4) {
        const f32x4 q = sq * scale, go = sg * gs;
        tq = pack4(q); tg = pack4(go);
        *reinterpret_cast<f32x4 *>(Qr + srr * PT + sc4) = tq;
        *reinterpret_cast<f32x4 *>(Gr + srr * PT + sc4) = tg;
        float dl = fmaf(go[0], so[0], fmaf(go[1], so[1], fmaf(go[2], so[2], go[3] * so[3])));
        dl += __shfl_xor(dl, 1, 64);
        dl += __shfl_xor(dl, 2, 64);
        dl += __shfl_xor(dl, 4, 64);
        dl += __shfl_xor(dl, 8, 64);
        if ((ss & 15) == 0) Dl[srr] = dl;
      }
    };
    auto stage_cols = [&]() {
      if (j < 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { Qt[(sc4 + i) * PTT + srr] = tq[i]; Gt[(sc4 + i) * PTT + srr] = tg[i]; }
      }
    };
    // dQ of the row tile from r0: the group's partials in the order of the waves, by the calling wave alone
    auto store_dq = [&](int r0) {
      const int row = r0 + fr;
      const bool st = row < g.N && live;
      float *out = dQKV + (ep + min(row, g.N - 1)) * 3 * d;
      const bool notkey = kidx[row] < 0;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {      // channels 16 ct + 4 g + r of row fr; zeros for the K / V gradient slices of the rows that are not keys
        f32x4 v = *reinterpret_cast<const f32x4 *>(Xq + (ct * 64 + lane) * 4);
#pragma unroll
        for (int jj = 1; jj < G; ++jj) v += *reinterpret_cast<const f32x4 *>(Xq + ((jj * NCT + ct) * 64 + lane) * 4);
        if (st) {
          const f32x4 o = v * (scale * ginv);
          track(o);
          *reinterpret_cast<f32x4 *>(out + qc + 16 * ct + 4 * fg) = o;
          if (notkey) {
            *reinterpret_cast<f32x4 *>(out + kc + 16 * ct + 4 * fg) = z4;
            *reinterpret_cast<f32x4 *>(out + vc + 16 * ct + 4 * fg) = z4;
          }
        }
      }
    };
    // ---- K / V of the wave's key tiles, once, in both operand layouts (attn_bwd_long.h) -------------------------------------------
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
      __builtin_amdgcn_sched_barrier(0);      // (the loads of one layout at a time: this prologue is the kernel's register peak otherwise)
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
        const H8 ks = split4(ka[ct]);
        const u2 hi = __builtin_bit_cast(u2, ks.hi), lo = __builtin_bit_cast(u2, ks.lo);
        *reinterpret_cast<f32x4 *>(Kt + ((t * NCT + ct) * 64 + lane) * 4) = (f32x4){__uint_as_float(hi[0]), __uint_as_float(hi[1]), __uint_as_float(lo[0]), __uint_as_float(lo[1])};
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) { dKT[t][ct] = z4; dVT[t][ct] = z4; }
    load_rows(0);
    put_rows();
    // ---- row tiles -----------------------------------------------------------------------------------------------------------------
    for (int rt = 0; rt < ntile; ++rt) {
      const int r0 = 16 * rt;
      __syncthreads();      // A
      stage_cols();
      if (rt > 0 && (rt - 1) % G == j) store_dq(r0 - 16);
      const int4 nv = *reinterpret_cast<const int4 *>(nvis + r0 + 4 * fg);
      const f32x4 dl4 = *reinterpret_cast<const f32x4 *>(Dl + 4 * fg);
      // S and dP of the wave's key tiles, the operands of a 16-channel step from the row-major image; the statistics of rows 4 g + r
      f32x4 S[TPW], dP[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) { S[t] = z4; dP[t] = z4; }
#pragma unroll
      for (int kg = 0; kg < NG; ++kg) {
        const H8 QA = unpack4(*reinterpret_cast<const f32x4 *>(Qr + fr * PT + 16 * kg + 4 * fg));
        const H8 GA = unpack4(*reinterpret_cast<const f32x4 *>(Gr + fr * PT + 16 * kg + 4 * fg));
#pragma unroll
        for (int t = 0; t < TPW; ++t)
          if (16 * (t * G + j) < n_ak) { mfma3(S[t], QA, KB[t][kg]); mfma3(dP[t], GA, VB[t][kg]); }
        __builtin_amdgcn_sched_barrier(0);      // (streamed: the operands of the next step are not hoisted over this one)
      }
      f32x4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int key = 16 * (t * G + j) + fr;
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
      if (rt + 1 < ntile) load_rows(r0 + 16);
      // the row's statistics over the group: M = max_j m_j, L = sum_j l_j exp(m_j - M), merged in the order j = 0 .. G - 1; this wave's factor exp(m - M) / L
      f32x4 fac;
      {
        f32x4 M = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, L = z4;
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {      // (merged pair by pair: one pair live instead of G; every wave runs the same order)
          const f32x4 a = *reinterpret_cast<const f32x4 *>(St + jj * 32 + 8 * fg), c = *reinterpret_cast<const f32x4 *>(St + jj * 32 + 8 * fg + 4);
          const float m[4] = {a[0], a[2], c[0], c[2]}, l[4] = {a[1], a[3], c[1], c[3]};
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (m[r] != -INFINITY) {
              const float Mn = fmaxf(M[r], m[r]);
              L[r] = L[r] * __expf(M[r] - Mn) + l[r] * __expf(m[r] - Mn);
              M[r] = Mn;
            }
          if (jj & 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) fac[r] = (mx[r] == -INFINITY || !(L[r] > 0.f)) ? 0.f : __expf(mx[r] - M[r]) / L[r];
      }
      // P, dS and dS^T (through the wave's transpose slot: write [row 4 g + r][key fr], read [row fr][keys 4 g .. 4 g + 3]) of each tile
      H8 PS[TPW], dSS[TPW], dST[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        f32x4 P, dS;
#pragma unroll
        for (int r = 0; r < 4; ++r) { P[r] = S[t][r] * fac[r]; dS[r] = P[r] * (dP[t][r] - dl4[r]); }
        PS[t] = split4(P); dSS[t] = split4(dS);
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(4 * fg + r) * 16 + fr] = dS[r];
        dST[t] = split4(*reinterpret_cast<const f32x4 *>(Ts + fr * 16 + 4 * fg));
      }
      // per 16 channels, the operands from the transposed image:  dV^T += dO^T P,  dK^T += Q^T dS,  dQ^T partial += K^T dS^T
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const H8 QTA = unpack4(*reinterpret_cast<const f32x4 *>(Qt + (16 * ct + fr) * PTT + 4 * fg));
        const H8 GTA = unpack4(*reinterpret_cast<const f32x4 *>(Gt + (16 * ct + fr) * PTT + 4 * fg));
        f32x4 dQT = z4;
#pragma unroll
        for (int t = 0; t < TPW; ++t)
          if (16 * (t * G + j) < n_ak) {
            mfma3(dVT[t][ct], GTA, PS[t]);
            mfma3(dKT[t][ct], QTA, dSS[t]);
            mfma3(dQT, tailbwd::as_h8(*reinterpret_cast<const f32x4 *>(Kt + ((t * NCT + ct) * 64 + lane) * 4)), dST[t]);
          }
        *reinterpret_cast<f32x4 *>(Xq + ((j * NCT + ct) * 64 + lane) * 4) = dQT;
        __builtin_amdgcn_sched_barrier(0);
      }
      if (rt + 1 < ntile) put_rows();
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

}  // namespace abwl64
