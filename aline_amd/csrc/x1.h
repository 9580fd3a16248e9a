// x1 path: d = 128 (4 heads of 32) at REFERENCE precision on the f16 matrix pipe -- the arithmetic, the tile images, the key list, the
// cyclic weight stream and the <= 64-key attention of x3_impl.h, with a weight layout and kernels of its own.
// (no include guard: x3_impl.h includes this file inside namespace x1, where X3_PAIRED is set, after its width-generic parts)
//
// Why its own layout: at d = 128 a k-step of a product is 8 output tiles, HALF a 16-pair chunk, so x3's "chunk = 16 output tiles of one
// k-step" does not exist.  Here
//   a D x D product is 2 chunks:        pair p of chunk c = k-step 2 c + (p >> 3), output tile p & 7;
//   32 hidden units are exactly 1 chunk: pairs 0 .. 7 = W1 (pair q: k-step q >> 1, hidden tile q & 1), pairs 8 .. 15 = W2 (output tile
//                                        p - 8, k-step = the group), so the hidden units are made in the middle of the chunk;
//   a head image packs two groups of 32 hidden units per chunk (pair p: group 2 ch + (p >> 3), then as W1 above).
// Why two tiles per wave: a 16-row tile is 32 registers of hi / lo fragments + 32 accumulators, so a 256-register wave carries TWO
// token tiles (64 + 64) beside the 64 registers of the fragment ring, and every weight fragment pair read from LDS feeds 6 MFMAs
// instead of 3 -- the LDS read rate per MFMA, which DESIGN 4.3's probe table names as the cap of the x3 loop, halves.  The two tiles
// of a wave are consecutive tiles of ONE episode (an odd last tile rides alone: its partner slot recomputes it and stores nothing), so
// the K / V fragments of a head are requested once and serve both.

// ---- weight image ---------------------------------------------------------------------------------------------------------------
constexpr int PC = 2;                                  // chunks of a D x D product
static_assert(D == 128 && NKS == 4 && NMT == 8 && KPH == 1 && MPH == 2 && WAVES == 8, "x1.h: d = 128, 4 heads of 32, 8 waves");
// layer image (32-bit words): chunks [Q 2][K 2][V 2][OUT 2][FFN F / 32], then the fp32 parameters of x3_impl.h's layer image
__host__ __device__ inline int layer_chunks(int F) { return 4 * PC + F / 32; }
__host__ __device__ inline int layer_params(int F) { return 9 * D + F; }
__host__ __device__ inline long layer_words(int F) { return (long)layer_chunks(F) * CHUNK_WORDS + layer_params(F); }
// head image (acquisition head, GMM heads): ceil(F / 64) chunks of W1 (an odd last group leaves half a chunk of zeros), then b1 [F] | w2 [3][F] | b2 [4]
__host__ __device__ inline int head_chunks(int F) { return (F / 32 + 1) / 2; }
__host__ __device__ inline int head_params(int F) { return 4 * F + 4; }
__host__ __device__ inline int head_lds_params(int F) { return 4 * F; }
__host__ __device__ inline long head_words(int F) { return (long)head_chunks(F) * CHUNK_WORDS + head_params(F); }
__host__ __device__ inline long image_words(int L, int F, int C) { return (long)L * layer_words(F) + (long)(1 + C) * head_words(F); }
// work units of the layer kernel: pairs of consecutive tiles of an episode
__host__ __device__ inline long layer_units(long B, int tpe) { return B * ((tpe + 1) / 2); }

__global__ void pack_kernel(PackArgs a) {
  const long lw = layer_words(a.F), hw = head_words(a.F), total = image_words(a.L, a.F, a.C);
  const float qscale = rsqrtf((float)HD) * 1.44269504088896340736f;   // softmax runs in exp2
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    unsigned v = 0;
    if (i < a.L * lw) {
      const int l = i / lw;
      const long o = i % lw, nfw = (long)layer_chunks(a.F) * CHUNK_WORDS;
      if (o < nfw) {
        const int ch = o / CHUNK_WORDS, cw = o % CHUNK_WORDS, p = cw >> 9, e = cw & 511;
        if (ch < 4 * PC) {
          const int mat = ch / PC, ks = 2 * (ch % PC) + (p >> 3), row0 = 16 * (p & 7);
          if (mat < 3) v = pair_word(a.in_proj_w[l] + (long)mat * D * D, D, row0, ks, e, (mat == 0 ? qscale : 1.f) * WSCALE, a.range_flag);
          else v = pair_word(a.out_proj_w[l], D, row0, ks, e, WSCALE, a.range_flag);
        } else {
          const int c = ch - 4 * PC;
          if (p < 8) v = pair_word(a.lin1_w[l], D, 32 * c + 16 * (p & 1), p >> 1, e, WSCALE, a.range_flag);
          else v = pair_word(a.lin2_w[l], a.F, 16 * (p - 8), c, e, WSCALE, a.range_flag);
        }
      } else {
        const int p = o - nfw;
        float f;
        if (p < 3 * D) f = a.in_proj_b[l][p] * (p < D ? qscale : 1.f);
        else if (p < 4 * D) f = a.out_proj_b[l][p - 3 * D];
        else if (p < 4 * D + a.F) f = a.lin1_b[l][p - 4 * D];
        else {
          const int q = p - 4 * D - a.F;
          f = q < D ? a.lin2_b[l][q] : q < 2 * D ? a.n1w[l][q - D] : q < 3 * D ? a.n1b[l][q - 2 * D]
            : q < 4 * D ? a.n2w[l][q - 3 * D] : a.n2b[l][q - 4 * D];
        }
        v = __float_as_uint(f);
      }
    } else {
      const long oh = i - a.L * lw;
      const int k = oh / hw;                          // 0: acquisition head, 1 + c: GMM head c
      const long o = oh % hw, nfw = (long)head_chunks(a.F) * CHUNK_WORDS;
      const float *w1 = k == 0 ? a.acq_w1 : a.gmm_w1[k - 1], *b1 = k == 0 ? a.acq_b1 : a.gmm_b1[k - 1];
      const float *w2 = k == 0 ? a.acq_w2 : a.gmm_w2[k - 1], *b2 = k == 0 ? a.acq_b2 : a.gmm_b2[k - 1];
      const int nout = k == 0 ? 1 : 3;
      const int ldw1 = D + ((k == 0 && a.time_token) ? 1 : 0);
      if (o < nfw) {
        const int ch = o / CHUNK_WORDS, cw = o % CHUNK_WORDS, p = cw >> 9, e = cw & 511, c = 2 * ch + (p >> 3), q = p & 7;
        if (32 * c < a.F) v = pair_word(w1, ldw1, 32 * c + 16 * (q & 1), q >> 1, e, WSCALE, a.range_flag);
      } else {
        const int p = o - nfw;
        float f = p < a.F ? b1[p] : p < (1 + nout) * a.F ? w2[p - a.F] : (p >= 4 * a.F && p < 4 * a.F + nout) ? b2[p - 4 * a.F] : 0.f;
        if (k == 0 && a.time_token && p >= 2 * a.F && p < 3 * a.F) f = w1[(long)(p - 2 * a.F) * ldw1 + D];      // the time column
        v = __float_as_uint(f);
      }
    }
    a.out[i] = v;
  }
}

// ---- K / V of the key rows: a workgroup computes K and V of 8 key tiles, one per wave (the 4 chunks of Wk | Wv per group) -----------
// Written as the A fragments the attention reads (x3_impl.h, KV_EP): K pairs [channel k-step][kt 4], V^T pairs [channel tile][s 2].
__global__ __launch_bounds__(THREADS) void kv_all_kernel(KvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *prm = reinterpret_cast<float *>(lds + NBUF * CHUNK_BYTES);      // bk | bv
  const int tid = threadIdx.x, lane = tid & 63, tok = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float *gprm = reinterpret_cast<const float *>(a.img + (long)layer_chunks(a.F) * CHUNK_WORDS);
  for (int i = tid; i < 2 * D; i += THREADS) prm[i] = gprm[D + i];
  const char *wbase = reinterpret_cast<const char *>(a.img) + (long)PC * CHUNK_BYTES;     // K chunks, then V chunks
  auto st = make_stream([wbase](int s) { return wbase + (long)s * CHUNK_BYTES; }, lds, 2 * PC, tid);
  st.start();
  __syncthreads();
  st.sync();
  FragRing ring;
  const long ntiles = (long)a.g.B * a.nkt2;
  for (int grp = blockIdx.x; grp < a.ngroups; grp += gridDim.x) {
    const long tile = (long)grp * WAVES + wave;
    const bool valid = tile < ntiles;
    const long tl = valid ? tile : ntiles - 1;
    const int b = tl / a.nkt2, kt = tl % a.nkt2, key = 16 * kt + tok;
    const bool live = key < a.kcnt[2 * b + 1];          // (slots behind the key count hold stale rows: zeroed, the attention masks them)
    f16x8 xh[NKS], xl[NKS];
    load_tile(a.X, (long)b * (WNK / 16) + kt, lane, xh, xl);
    if (!live) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) { xh[ks] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0}; xl[ks] = xh[ks]; }
    }
    u32x4 *kv = a.KV + (long)b * KV_EP;
    f32x4 y[NMT];
    // K^T = Wk KX^T: rows = channels, columns = keys -> A fragments of S^T = K Q^T, pair (channel k-step = head h, kt)
#pragma unroll
    for (int m = 0; m < NMT; ++m) y[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chunk_run<PC>(st, ring, [&](int cc, int p, const f16x8 &ah, const f16x8 &al) { mfma3(y[p & 7], ah, al, xh[2 * cc + (p >> 3)], xl[2 * cc + (p >> 3)]); });
#pragma unroll
    for (int h = 0; h < NKS; ++h) {
      const f32x4 b0 = *reinterpret_cast<const f32x4 *>(prm + 32 * h + 4 * g), b1 = *reinterpret_cast<const f32x4 *>(prm + 32 * h + 16 + 4 * g);
      f16x8 fh, fl;
      split_frag(y[2 * h] * WINV + b0, y[2 * h + 1] * WINV + b1, fh, fl);
      if (valid) {
        kv[((h * 4 + kt) * 2) * 64 + lane] = __builtin_bit_cast(u32x4, fh);
        kv[((h * 4 + kt) * 2 + 1) * 64 + lane] = __builtin_bit_cast(u32x4, fl);
      }
    }
    // V = KX Wv^T with the MFMA operands swapped (rows = keys, columns = channels): accumulator tile i holds
    // V[key 16 kt + 4 g + r][channel 16 i + tok] -- half (kt & 1) of this lane's piece of the V^T pair (i, kt / 2)
#pragma unroll
    for (int m = 0; m < NMT; ++m) y[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chunk_run<PC>(st, ring, [&](int cc, int p, const f16x8 &bh, const f16x8 &bl) { mfma3(y[p & 7], xh[2 * cc + (p >> 3)], xl[2 * cc + (p >> 3)], bh, bl); });
#pragma unroll
    for (int i = 0; i < NMT; ++i) {
      const float bv = prm[D + 16 * i + tok];
      unsigned h0, l0, h1, l1;
      split2(y[i][0] * WINV + bv, y[i][1] * WINV + bv, h0, l0);
      split2(y[i][2] * WINV + bv, y[i][3] * WINV + bv, h1, l1);
      if (valid) {
        u32x2 *ph = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (kt >> 1)) * 2) * 64 + lane) + (kt & 1);
        u32x2 *pl = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (kt >> 1)) * 2 + 1) * 64 + lane) + (kt & 1);
        *ph = (u32x2){h0, h1};
        *pl = (u32x2){l0, l1};
      }
    }
  }
  st.finish();
}

// ---- the two-tile chunk pipeline ------------------------------------------------------------------------------------------------
// acc0 += A X0, acc1 += A X1 for one weight pair A: the three terms of the two tiles alternate, so that no MFMA waits for the one
// issued just before it (each accumulator still sums its terms in mfma3's order: small terms first)
__device__ __forceinline__ void mfma3x2(f32x4 &acc0, f32x4 &acc1, const f16x8 &ah, const f16x8 &al, const f16x8 &b0h, const f16x8 &b0l,
                                        const f16x8 &b1h, const f16x8 &b1l) {
  XMFMA(acc0, al, b0h); XMFMA(acc1, al, b1h);
  XMFMA(acc0, ah, b0l); XMFMA(acc1, ah, b1l);
  XMFMA(acc0, ah, b0h); XMFMA(acc1, ah, b1h);
}
// One chunk, as chunk_pipe, with exactly 6 MFMAs per pair (body(p, A_hi, A_lo): both tiles) -- 24 per batch of 4 pairs behind the same
// 8 fragment reads and 4 LDS-DMA pieces.  mid() runs in front of batch MID (MID < 0: never): the hidden units of an FFN chunk, between
// its W1 half and its W2 half.  Same preconditions and the same end (the sync() of the next chunk) as chunk_pipe.
template <bool PREFETCH_NEXT, int MID, class St, class Body, class Mid>
__device__ __forceinline__ void pair_pipe(St &st, FragRing &r, const f16x8 *cur, const f16x8 *nxt, Body body, Mid mid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    __builtin_amdgcn_sched_barrier(0);
    touch_batch(r, k & 1);
    __builtin_amdgcn_sched_barrier(0);
    if (k == MID) {
      mid();
      __builtin_amdgcn_sched_barrier(0);
    }
    const bool reads = k < 3 || PREFETCH_NEXT;
    if (k < 3) fetch_batch(r, (k + 1) & 1, cur, k + 1);
    else if (PREFETCH_NEXT) fetch_batch(r, 0, nxt, 0);
    if (k == st.dma_slot) st.issue();
#pragma unroll
    for (int j = 0; j < 4; ++j) body(4 * k + j, r.hi[k & 1][j], r.lo[k & 1][j]);
#define X1_MFMA(n) __builtin_amdgcn_sched_group_barrier(0x008, n, 0)
#define X1_READ(n) __builtin_amdgcn_sched_group_barrier(0x100, n, 0)
#define X1_DMA1() __builtin_amdgcn_sched_group_barrier(0x020, 1, 0)
    if (k != st.dma_slot) {                            // a read behind each of the first eight MFMAs
      if (reads) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { X1_MFMA(1); X1_READ(1); }
        X1_MFMA(16);
      } else {
        X1_MFMA(24);
      }
    } else {                                           // two reads behind each of four MFMAs, then the wave's pieces of the stream
#pragma unroll
      for (int i = 0; i < 4; ++i) { X1_MFMA(1); if (reads) X1_READ(2); }
#pragma unroll
      for (int i = 0; i < PIECES_PER_WAVE; ++i) { X1_MFMA(1); X1_DMA1(); }
      X1_MFMA(20 - PIECES_PER_WAVE);
    }
#undef X1_MFMA
#undef X1_READ
#undef X1_DMA1
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_sched_barrier(0);
  st.sync();
}
// The two chunks of a D x D product: pair p of chunk i is consumed by body(i, p, A_hi, A_lo), hook(i) runs behind chunk i
template <class St, class Body, class Hook>
__device__ __forceinline__ void pair_product(St &st, FragRing &r, Body body, Hook hook) {
  prime(r, st.cur());
#pragma unroll
  for (int i = 0; i < PC; ++i) {
    const f16x8 *cur = st.cur(), *nx = st.nxt();
    st.advance();
    auto bi = [&](int p, const f16x8 &ah, const f16x8 &al) { body(i, p, ah, al); };
    if (i + 1 < PC) pair_pipe<true, -1>(st, r, cur, nx, bi, [] {});
    else pair_pipe<false, -1>(st, r, cur, nx, bi, [] {});
    hook(i);
  }
}

// masked set-attention of the two tiles of a wave against NKT key tiles of their episode, head by head: attention_tile's arithmetic
// per tile, with ONE request of a head's K / V fragment pairs (the head after the one being computed) serving both tiles.  The tiles
// of a head run one after the other (16 scores live, not 32), and the visibility mask is recomputed per head from nv[t] instead of
// being kept (attention_long's trade): 2 x 64 registers of K / V pairs + 64 of Q^T fragments leave no room for either.
template <int NKT>
__device__ __forceinline__ void attention_pair(f16x8 (&qh)[2][NKS], f16x8 (&ql)[2][NKS], const u32x4 *kv, const int (&nv)[2], HeadKV<NKT> &first) {
  constexpr int NS = NKT > 2 ? 2 : 1;
  const float inf = opaque_inf();
  HeadKV<NKT> buf[2];
  buf[0] = first;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    HeadKV<NKT> &c = buf[h & 1];
    if (h + 1 < H) buf[(h + 1) & 1].load(kv, h + 1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int nvh = nv[t];
      asm volatile("" : "+v"(nvh));                     // (opaque: the mask values are recomputed, not carried from head to head)
      f32x4 s[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = (16 * kt + r) < nvh ? 0.f : -INFINITY;
        mfma3(s[kt], __builtin_bit_cast(f16x8, c.k[2 * kt]), __builtin_bit_cast(f16x8, c.k[2 * kt + 1]), qh[t][h], ql[t][h]);
      }
      float mx = vmax(vmax(s[0][0], s[0][1], inf), vmax(s[0][2], s[0][3], inf), inf);
#pragma unroll
      for (int kt = 1; kt < NKT; ++kt) mx = vmax(mx, vmax(vmax(s[kt][0], s[kt][1], inf), vmax(s[kt][2], s[kt][3], inf), inf), inf);
      mx = group_max4(mx, inf);
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - mx);
          sum += s[kt][r];
        }
      const float inv = __builtin_amdgcn_rcpf(group_sum4(sum));                          // (v_rcp_f32: 1 ulp)
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 o[MPH] = {z4, z4};
#pragma unroll
      for (int si = 0; si < NS; ++si) {
        f16x8 ph, pl;
        split_frag(s[2 * si], (2 * si + 1 < NKT) ? s[(2 * si + 1 < NKT) ? 2 * si + 1 : 0] : z4, ph, pl);
#pragma unroll
        for (int ii = 0; ii < MPH; ++ii)
          mfma3(o[ii], __builtin_bit_cast(f16x8, c.v[(ii * NS + si) * 2]), __builtin_bit_cast(f16x8, c.v[(ii * NS + si) * 2 + 1]), ph, pl);
      }
      split_frag(o[0] * inv, o[1] * inv, qh[t][h], ql[t][h]);
    }
  }
}

// layer_kernel<LAST> (the rollout) and layer_save_kernel (the training backward's forward recompute): one text, two passes
#define X1_SAVE 0
#include "x1_layer.h"
#undef X1_SAVE
#define X1_SAVE 1
#include "x1_layer.h"
#undef X1_SAVE

// ---- acquisition head (NOUT = 1) / one GMM head (NOUT = 3): x3's head kernel on the two-groups-per-chunk head image ------------------
// out[row * out_stride + out_off + j] = w2[j] . relu(W1 z + b1) + b2[j] over the 16-row tiles of an image, one tile per wave
template <int NOUT>
__global__ __launch_bounds__(THREADS) void head_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *prm = reinterpret_cast<float *>(lds + NBUF * CHUNK_BYTES);      // b1 [F] | w2 [3][F]
  const int tid = threadIdx.x, lane = tid & 63, tok = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = a.F;
  const float *gprm = reinterpret_cast<const float *>(a.img + (long)head_chunks(F) * CHUNK_WORDS);
  for (int i = tid; i < head_lds_params(F); i += THREADS) prm[i] = (a.tau != 0.f && i < F) ? fmaf(a.tau, gprm[2 * F + i], gprm[i]) : gprm[i];
  const char *wbase = reinterpret_cast<const char *>(a.img);
  auto st = make_stream([wbase](int s) { return wbase + (long)s * CHUNK_BYTES; }, lds, head_chunks(F), tid);
  st.start();
  __syncthreads();
  st.sync();
  FragRing ring;
  for (int grp = blockIdx.x; grp < a.ngroups; grp += gridDim.x) {
    const long tile = (long)grp * WAVES + wave;
    const bool valid = tile < a.ntiles;
    const long tl = valid ? tile : a.ntiles - 1;
    const long row = 16 * tl + tok;
    f16x8 xh[NKS], xl[NKS];
    load_tile(a.X, tl, lane, xh, xl);
    float plog[NOUT];
#pragma unroll
    for (int jo = 0; jo < NOUT; ++jo) plog[jo] = 0.f;
    prime(ring, st.cur());
#pragma unroll 1
    for (int ch = 0; ch < head_chunks(F); ++ch) {
      f32x4 h[4];                                       // [group of the chunk][hidden tile]
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const f16x8 *cur = st.cur(), *nx = st.nxt();
      st.advance();
      chunk_pipe<true>(st, ring, cur, nx, [&](int p, const f16x8 &ah, const f16x8 &al) {
        mfma3(h[2 * (p >> 3) + (p & 1)], ah, al, xh[(p & 7) >> 1], xl[(p & 7) >> 1]);
      });
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int c = 2 * ch + half;
        if (32 * c < F) {                               // (an odd F / 32: the last chunk's second group is zeros and counts for nothing)
          const f32x4 c0 = *reinterpret_cast<const f32x4 *>(prm + 32 * c + 4 * g), c1 = *reinterpret_cast<const f32x4 *>(prm + 32 * c + 16 + 4 * g);
          const f32x4 h0 = h[2 * half] * WINV + c0, h1 = h[2 * half + 1] * WINV + c1;
#pragma unroll
          for (int jo = 0; jo < NOUT; ++jo) {
            const f32x4 w0 = *reinterpret_cast<const f32x4 *>(prm + (1 + jo) * F + 32 * c + 4 * g);
            const f32x4 w1 = *reinterpret_cast<const f32x4 *>(prm + (1 + jo) * F + 32 * c + 16 + 4 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              plog[jo] = fmaf(relu_nn(h0[q]), w0[q], plog[jo]);
              plog[jo] = fmaf(relu_nn(h1[q]), w1[q], plog[jo]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int jo = 0; jo < NOUT; ++jo) {
      const float v = group_sum4(plog[jo]) + gprm[4 * F + jo];
      if (g == 0 && valid && row < a.M) a.out[row * a.out_stride + a.out_off + jo] = v;
    }
  }
  st.finish();
}
