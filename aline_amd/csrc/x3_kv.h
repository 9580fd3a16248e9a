// K / V of the key rows (kernels of x3_impl.h; no include guard: x3_impl.h includes this file once per key layout, with X3_KV_LONG set)
//   X3_KV_LONG 0: kv_all_kernel / kv_split_kernel -- an episode's keys in ONE block of the KV_EP layout (up to WNK keys)
//   X3_KV_LONG 1: kv_all_long_kernel / kv_split_long_kernel -- the long-key layout, `ktiles` = 4 groups key tiles per episode: key tile kt
//                 in block kt >> 2 at index kt & 3 (its V^T k-step: index (kt & 3) >> 1, half kt & 1, as in the one-block layout)
#if X3_KV_LONG
#define X3_KV_KERNEL(name) X3_NO_PK_F32 name##_long_kernel(KvArgs a, int ktiles)
#define X3_KV_KTILES ktiles
#define X3_KV_BLOCK(b, kt) ((long)(b) * (ktiles >> 2) + ((kt) >> 2))
#define X3_KV_KQ(kt) ((kt) & 3)
#else
#define X3_KV_KERNEL(name) name##_kernel(KvArgs a)
#define X3_KV_KTILES (WNK / 16)
#define X3_KV_BLOCK(b, kt) (long)b
#define X3_KV_KQ(kt) kt
#endif

// A workgroup computes K and V of its group of WAVES key tiles (all 2 PC chunks of Wk | Wv per group).
__global__ __launch_bounds__(THREADS) void X3_KV_KERNEL(kv_all) {
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
    load_tile(a.X, (long)b * X3_KV_KTILES + kt, lane, xh, xl);
    if (!live) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) { xh[ks] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0}; xl[ks] = xh[ks]; }
    }
    u32x4 *kv = a.KV + X3_KV_BLOCK(b, kt) * KV_EP;
    f32x4 y[NMT];
    // K^T = Wk KX^T: rows = channels, columns = keys -> A fragments of S^T = K Q^T, pair (channel k-step h, kt) -- a head is KPH k-steps
#pragma unroll
    for (int m = 0; m < NMT; ++m) y[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chunk_run<PC>(st, ring, [&](int cc, int p, const f16x8 &ah, const f16x8 &al) { mfma3(y[16 * (cc % CPK) + p], ah, al, xh[cc / CPK], xl[cc / CPK]); });
#pragma unroll
    for (int h = 0; h < NKS; ++h) {
      const f32x4 b0 = *reinterpret_cast<const f32x4 *>(prm + 32 * h + 4 * g), b1 = *reinterpret_cast<const f32x4 *>(prm + 32 * h + 16 + 4 * g);
      f16x8 fh, fl;
      split_frag(y[2 * h] * WINV + b0, y[2 * h + 1] * WINV + b1, fh, fl);
      if (valid) {
        kv[((h * 4 + X3_KV_KQ(kt)) * 2) * 64 + lane] = __builtin_bit_cast(u32x4, fh);
        kv[((h * 4 + X3_KV_KQ(kt)) * 2 + 1) * 64 + lane] = __builtin_bit_cast(u32x4, fl);
      }
    }
    // V = KX Wv^T with the MFMA operands swapped (rows = keys, columns = channels): accumulator tile i holds
    // V[key 16 kt + 4 g + r][channel 16 i + tok] -- half (kt & 1) of this lane's piece of the V^T pair (i, kt / 2)
#pragma unroll
    for (int m = 0; m < NMT; ++m) y[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chunk_run<PC>(st, ring, [&](int cc, int p, const f16x8 &bh, const f16x8 &bl) { mfma3(y[16 * (cc % CPK) + p], xh[cc / CPK], xl[cc / CPK], bh, bl); });
#pragma unroll
    for (int i = 0; i < NMT; ++i) {
      const float bv = prm[D + 16 * i + tok];
      unsigned h0, l0, h1, l1;
      split2(y[i][0] * WINV + bv, y[i][1] * WINV + bv, h0, l0);
      split2(y[i][2] * WINV + bv, y[i][3] * WINV + bv, h1, l1);
      if (valid) {
        u32x2 *ph = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (X3_KV_KQ(kt) >> 1)) * 2) * 64 + lane) + (kt & 1);
        u32x2 *pl = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (X3_KV_KQ(kt) >> 1)) * 2 + 1) * 64 + lane) + (kt & 1);
        *ph = (u32x2){h0, h1};
        *pl = (u32x2){l0, l1};
      }
    }
  }
  st.finish();
}

// The same split into jobs -- (K | V) x (CPK halves of the D output channels): 16 output tiles and NKS chunks each --, one job per
// workgroup (blockIdx % (2 CPK)), for launches with fewer groups of key tiles than CUs: at d = 512 / B = 256 there are 128 groups, each
// streaming 2 MB of weights through one CU's LDS-DMA (60 us per launch, 14 % of the cfg5 rollout); split four ways every CU streams.
__global__ __launch_bounds__(THREADS) void X3_KV_KERNEL(kv_split) {
  constexpr bool SPLIT = true;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *prm = reinterpret_cast<float *>(lds + NBUF * CHUNK_BYTES);      // bk | bv
  const int tid = threadIdx.x, lane = tid & 63, tok = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float *gprm = reinterpret_cast<const float *>(a.img + (long)layer_chunks(a.F) * CHUNK_WORDS);
  for (int i = tid; i < 2 * D; i += THREADS) prm[i] = gprm[D + i];
  constexpr int NJ = 2 * CPK;
  const int job0 = SPLIT ? (int)(blockIdx.x % NJ) : 0;
  const int grp0 = SPLIT ? (int)(blockIdx.x / NJ) : (int)blockIdx.x, gstride = SPLIT ? (int)(gridDim.x / NJ) : (int)gridDim.x;
  const char *wbase = reinterpret_cast<const char *>(a.img) + (long)PC * CHUNK_BYTES;     // K chunks, then V chunks
  // stream position s -> job (SPLIT: job0; else s / NKS), k-step s % NKS -> chunk (K | V) PC + CPK k + half
  auto st = make_stream([wbase, job0](int s) {
    const int job = SPLIT ? job0 : s / NKS, k = s % NKS;
    return wbase + (long)((job / CPK) * PC + CPK * k + job % CPK) * CHUNK_BYTES;
  }, lds, (SPLIT ? 1 : NJ) * NKS, tid);
  st.start();
  __syncthreads();
  st.sync();
  FragRing ring;
  const long ntiles = (long)a.g.B * a.nkt2;
  for (int grp = grp0; grp < a.ngroups; grp += gstride) {
    const long tile = (long)grp * WAVES + wave;
    const bool valid = tile < ntiles;
    const long tl = valid ? tile : ntiles - 1;
    const int b = tl / a.nkt2, kt = tl % a.nkt2, key = 16 * kt + tok;
    const bool live = key < a.kcnt[2 * b + 1];          // (slots behind the key count hold stale rows: zeroed, the attention masks them)
    f16x8 xh[NKS], xl[NKS];
    load_tile(a.X, (long)b * X3_KV_KTILES + kt, lane, xh, xl);
    if (!live) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) { xh[ks] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0}; xl[ks] = xh[ks]; }
    }
    u32x4 *kv = a.KV + X3_KV_BLOCK(b, kt) * KV_EP;
#pragma unroll
    for (int job = 0; job < NJ; ++job) {      // (unrolled: the job, and with it every register index and parameter offset, is a constant)
      if (SPLIT && job != job0) continue;
      const int half = job % CPK;
      f32x4 y[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) y[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (job < CPK) {
        // K^T = Wk KX^T: rows = channels, columns = keys -> A fragments of S^T = K Q^T, pair (channel k-step f, kt) -- a head is KPH k-steps
        chunk_run<NKS>(st, ring, [&](int cc, int p, const f16x8 &ah, const f16x8 &al) { mfma3(y[p], ah, al, xh[cc], xl[cc]); });
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int f = 8 * half + j;
          const f32x4 b0 = *reinterpret_cast<const f32x4 *>(prm + 32 * f + 4 * g), b1 = *reinterpret_cast<const f32x4 *>(prm + 32 * f + 16 + 4 * g);
          f16x8 fh, fl;
          split_frag(y[2 * j] * WINV + b0, y[2 * j + 1] * WINV + b1, fh, fl);
          if (valid) {
            kv[((f * 4 + X3_KV_KQ(kt)) * 2) * 64 + lane] = __builtin_bit_cast(u32x4, fh);
            kv[((f * 4 + X3_KV_KQ(kt)) * 2 + 1) * 64 + lane] = __builtin_bit_cast(u32x4, fl);
          }
        }
      } else {
        // V = KX Wv^T with the MFMA operands swapped (rows = keys, columns = channels): accumulator tile i holds
        // V[key 16 kt + 4 g + r][channel 16 i + tok] -- half (kt & 1) of this lane's piece of the V^T pair (i, kt / 2)
        chunk_run<NKS>(st, ring, [&](int cc, int p, const f16x8 &bh, const f16x8 &bl) { mfma3(y[p], xh[cc], xl[cc], bh, bl); });
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int i = 16 * half + j;
          const float bv = prm[D + 16 * i + tok];
          unsigned h0, l0, h1, l1;
          split2(y[j][0] * WINV + bv, y[j][1] * WINV + bv, h0, l0);
          split2(y[j][2] * WINV + bv, y[j][3] * WINV + bv, h1, l1);
          if (valid) {
            u32x2 *ph = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (X3_KV_KQ(kt) >> 1)) * 2) * 64 + lane) + (kt & 1);
            u32x2 *pl = reinterpret_cast<u32x2 *>(kv + KV_VOFF + ((i * 2 + (X3_KV_KQ(kt) >> 1)) * 2 + 1) * 64 + lane) + (kt & 1);
            *ph = (u32x2){h0, h1};
            *pl = (u32x2){l0, l1};
          }
        }
      }
    }
  }
  st.finish();
}

#undef X3_KV_KERNEL
#undef X3_KV_KTILES
#undef X3_KV_BLOCK
#undef X3_KV_KQ
