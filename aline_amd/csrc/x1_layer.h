// ---- one encoder layer of the two token tiles of a wave -------------------------------------------------------------------------------
// Q projection, masked set-attention, out-projection, LN1, FFN, LN2 in registers, as x3's layer kernel, for the tiles 2 j and 2 j + 1
// of an episode (unit u = episode * ceil(tpe / 2) + j).  Persistent workgroups of 8 waves walk the unit list in x3's rounds (full rounds
// of 8 units per workgroup, the rest spread over all workgroups); the cyclic weight stream of a round is Q (2 chunks), OUT (2), FFN
// (F / 32).  A wave without a unit in the last round keeps its share of the stream and the barriers going (idle_chunks).
// (no include guard: x1.h includes this file twice.  X1_SAVE 0: layer_kernel<LAST>, the rollout's kernel.  X1_SAVE 1: layer_save_kernel,
// the forward recompute of the per-op backward -- the same layer over the (step, episode) instances of a chunk, plus the fp32 rows
// LayerArgs.sv* of both tiles, straight from the accumulator layout: a lane holds features 16 m + 4 g + (0..3) of its token in y[t][m], so
// every store is 16 bytes of one row.  A store address is formed where it is used, from the scalar base pointer and the lane's row
// srow(t); whatever keeps a lane from storing its image rows keeps it from storing these (rowok[t]: rows >= N of a partial tile, and the
// partner slot of an odd last tile).  The variants are preprocessor passes, not a template parameter, so that the rollout's kernels are
// compiled from exactly the text they had -- their register allocation moves with dead code around it.)
#if X1_SAVE
// (x3's lever for the register fit, the per-kernel no-packed-fp32 attribute X3_NO_PK_F32, was tried first and is NOT used: with it the
//  kernel spills 99 registers / 384 bytes of scratch, without it 83 / 336 -- fewer than the rollout's kernels, two waves per SIMD either way)
__global__ __launch_bounds__(THREADS) void layer_save_kernel(LayerArgs a) {
  constexpr bool LAST = false;                          // (every layer files its key rows into the next layer's key image; no target image)
#else
template <bool LAST>
__global__ __launch_bounds__(THREADS) void layer_kernel(LayerArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *prm = reinterpret_cast<float *>(lds + NBUF * CHUNK_BYTES);   // bq bk bv | bo | b1 | b2 | ln1w ln1b ln2w ln2b
  const Geo &G = a.g;
  const int tid = threadIdx.x, lane = tid & 63, tok = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = a.F, np = layer_params(F), n_t = G.n_td + G.n_th;
  {
    const float *gprm = reinterpret_cast<const float *>(a.img + (long)layer_chunks(F) * CHUNK_WORDS);
    for (int i = tid; i < np; i += THREADS) prm[i] = gprm[i];
  }
  const LaneParams P = lane_params(prm, g);
  const int o_bo = 3 * D, o_b1 = 4 * D, o_b2 = o_b1 + F, o_ln1w = o_b2 + D, o_ln1b = o_ln1w + D, o_ln2w = o_ln1b + D, o_ln2b = o_ln2w + D;   // word offsets
  const char *wbase = reinterpret_cast<const char *>(a.img);
  const int seq = 2 * PC + F / 32;
  auto st = make_stream([wbase](int s) { return wbase + (long)(s < PC ? s : s + 2 * PC) * CHUNK_BYTES; }, lds, seq, tid);
  st.start();
  __syncthreads();
  st.sync();
  FragRing ring;
  float range_chk = 0.f;
  const int ppe = (a.tpe + 1) >> 1;                                            // units (tile pairs) of an episode
  const long nunits = layer_units(G.B, a.tpe);
  const int NG = gridDim.x;
  const long per_round = (long)NG * WAVES;
  const int full = (int)(nunits / per_round);
  const long rem = nunits - (long)full * per_round;
  const int ktail = (int)((rem + NG - 1) / NG);
  const bool wg_tail = rem > 0 && (long)blockIdx.x * ktail < rem;              // (workgroup-uniform) a tail round for this workgroup
  const long tail_unit = (long)full * per_round + (long)blockIdx.x * ktail + wave;
  const bool my_tail = wg_tail && wave < ktail && tail_unit < nunits;
  const int my_rounds = full + (my_tail ? 1 : 0);                              // rounds in which this wave computes a unit
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (int rd = 0; rd < my_rounds; ++rd) {
    const long unit = rd < full ? ((long)rd * NG + blockIdx.x) * WAVES + wave : tail_unit;
    const int b = (int)(unit / ppe), j2 = 2 * (int)(unit % ppe);
    const bool has1 = j2 + 1 < a.tpe;                                          // (wave-uniform) else the episode's odd last tile, twice
    long tl[2];
    int r[2], lidx[2], nv[2];
    bool rowok[2];
    const int n_ck = a.kcnt[2 * b], n_ak = a.kcnt[2 * b + 1];
    f16x8 xh[2][NKS], xl[2][NKS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int jt = j2 + ((t && has1) ? 1 : 0);
      tl[t] = (long)b * a.tpe + jt;
      r[t] = 16 * jt + tok;
      const int rc = min(r[t], G.N - 1);
      rowok[t] = r[t] < G.N && (t == 0 || has1);
      lidx[t] = 16 * g + (rc & 15);
      const bool isq = rc < G.P && !is_ctx(G, b, rc);
      nv[t] = (isq ? n_ak : n_ck) - 4 * g;              // key 16 kt + 4 g + r is visible iff 16 kt + r < nv
      load_tile(a.XIN, tl[t], lidx[t], xh[t], xl[t]);
    }
    const u32x4 *kv = a.KV + (long)b * KV_EP + lane;
    const int nkt = __builtin_amdgcn_readfirstlane((n_ak + 15) >> 4);     // (uniform per wave: one episode per unit)
#if X1_SAVE
    auto srow = [&](int t) -> long { return (long)b * G.N + min(r[t], G.N - 1); };      // fp32 row of this lane's token of tile t
    auto save_rows = [&](float *dst, int t, const f32x4 (&v)[NMT]) {
      if (rowok[t]) {
        float *p = dst + srow(t) * D + 4 * g;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) sv_store(p + 16 * mt, v[mt]);
      }
    };
#endif

    f32x4 y[2][NMT];
    auto clear_y = [&]() {
#pragma unroll
      for (int m = 0; m < NMT; ++m) { y[0][m] = z4; y[1][m] = z4; }
    };
    // ---- Q^T = Wq X^T (pre-scaled by log2(e) / sqrt(hd)) ----------------------------------------------------------
    clear_y();
    pair_product(st, ring, [&](int cc, int p, const f16x8 &ah, const f16x8 &al) {
      const int ks = 2 * cc + (p >> 3), m = p & 7;
      mfma3x2(y[0][m], y[1][m], ah, al, xh[0][ks], xl[0][ks], xh[1][ks], xl[1][ks]);
    }, [](int) {});
    // ---- attention: context and target rows see the context keys, query rows also the visible targets -------------
    f16x8 qh[2][NKS], ql[2][NKS];      // Q^T fragment pairs by head, then the attention output's
    auto q_epilogue = [&]() {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < NKS; ++h) {
          const f32x4 c0 = P(32 * h), c1 = P(32 * h + 16);
#if X1_SAVE
          if (rowok[t]) {
            constexpr float QINV = 5.65685424949238f * 0.69314718055994531f;      // sqrt(HD) / log2(e): undoes pack_kernel's qscale
            float *qp = a.svQ + srow(t) * a.svQ_ld + 32 * h + 4 * g;
            sv_store(qp, (y[t][2 * h] * WINV + c0) * QINV);
            sv_store(qp + 16, (y[t][2 * h + 1] * WINV + c1) * QINV);
          }
#endif
          split_frag(y[t][2 * h] * WINV + c0, y[t][2 * h + 1] * WINV + c1, qh[t][h], ql[t][h]);
        }
    };
    // (head 0's K / V pairs are requested before the epilogue of the Q projection and land while it runs)
    if (nkt <= 1) { HeadKV<1> k0; k0.load(kv, 0); q_epilogue(); attention_pair<1>(qh, ql, kv, nv, k0); }
    else if (nkt == 2) { HeadKV<2> k0; k0.load(kv, 0); q_epilogue(); attention_pair<2>(qh, ql, kv, nv, k0); }
    else { HeadKV<4> k0; k0.load(kv, 0); q_epilogue(); attention_pair<4>(qh, ql, kv, nv, k0); }
#if X1_SAVE
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (rowok[t]) {
        float *ap = a.svA + srow(t) * D + 4 * g;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          sv_store(ap + 32 * ks, frag_value(qh[t][ks], ql[t][ks], 0));
          sv_store(ap + 32 * ks + 16, frag_value(qh[t][ks], ql[t][ks], 1));
        }
      }
#endif
    // ---- X1 = LN1(X + bo + Wo A): the residual X comes back from L2 two k-steps per chunk, into the registers the consumed
    // fragments of the attention output free ----------------------------------------------------------------------------
    clear_y();
    pair_product(st, ring, [&](int cc, int p, const f16x8 &ah, const f16x8 &al) {
      const int ks = 2 * cc + (p >> 3), m = p & 7;
      mfma3x2(y[0][m], y[1][m], ah, al, qh[0][ks], ql[0][ks], qh[1][ks], ql[1][ks]);
    }, [&](int cc) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 2 * cc; ks < 2 * cc + 2; ++ks) {
          xh[t][ks] = __builtin_bit_cast(f16x8, a.XIN[xpiece(tl[t], ks, 0, lidx[t])]);
          xl[t][ks] = __builtin_bit_cast(f16x8, a.XIN[xpiece(tl[t], ks, 1, lidx[t])]);
        }
    });
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
        y[t][mt] = y[t][mt] * WINV + P(o_bo + 16 * mt) + frag_value(xh[t][mt >> 1], xl[t][mt >> 1], mt & 1);
#if X1_SAVE
      save_rows(a.svU1, t, y[t]);
#endif
      range_chk += layer_norm(y[t], P, o_ln1w, o_ln1b);
#if X1_SAVE
      save_rows(a.svX1, t, y[t]);
#endif
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) split_frag(y[t][2 * ks], y[t][2 * ks + 1], xh[t][ks], xl[t][ks]);
    }
    // ---- X = LN2(X1 + b2 + W2 relu(W1 X1 + b1)): 32 hidden units per chunk -- W1 in its first two batches, W2 in the other two ------
    clear_y();
    {
      f16x8 hbh[2], hbl[2];
      prime(ring, st.cur());
#pragma unroll 1
      for (int c = 0; c < F / 32; ++c) {
        f32x4 h[2][2] = {{z4, z4}, {z4, z4}};
        const f16x8 *cur = st.cur(), *nx = st.nxt();
        st.advance();
        pair_pipe<true, 2>(st, ring, cur, nx, [&](int p, const f16x8 &ah, const f16x8 &al) {
          if (p < 8) mfma3x2(h[0][p & 1], h[1][p & 1], ah, al, xh[0][p >> 1], xl[0][p >> 1], xh[1][p >> 1], xl[1][p >> 1]);
          else mfma3x2(y[0][p - 8], y[1][p - 8], ah, al, hbh[0], hbl[0], hbh[1], hbl[1]);
        }, [&]() {
          const f32x4 c0 = P(o_b1 + 32 * c), c1 = P(o_b1 + 32 * c + 16);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            f32x4 h0 = h[t][0] * WINV + c0, h1 = h[t][1] * WINV + c1;
#pragma unroll
            for (int q = 0; q < 4; ++q) { h0[q] = relu_nn(h0[q]); h1[q] = relu_nn(h1[q]); }
#if X1_SAVE
            if (rowok[t]) {      // (in front of the chunk's W2 batches: the stores drain while they run)
              float *hp = a.svHid + srow(t) * F + 32 * c + 4 * g;
              sv_store(hp, h0);
              sv_store(hp + 16, h1);
            }
#endif
            split_frag(h0, h1, hbh[t], hbl[t]);
          }
        });
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
        y[t][mt] = y[t][mt] * WINV + P(o_b2 + 16 * mt) + frag_value(xh[t][mt >> 1], xl[t][mt >> 1], mt & 1);
#if X1_SAVE
      save_rows(a.svU2, t, y[t]);
#endif
      range_chk += layer_norm(y[t], P, o_ln2w, o_ln2b);
#if X1_SAVE
      save_rows(a.svY, t, y[t]);
#endif
      const bool ztgt = LAST && a.zimg && rowok[t] && r[t] >= G.P;
      const long zr = a.zrow0 + (long)b * n_t + (r[t] - G.P);
      const int kp = (!LAST && rowok[t]) ? a.keypos[(long)b * 16 * a.tpe + r[t]] : -1;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        f16x8 oh, ol;
        split_frag(y[t][2 * ks], y[t][2 * ks + 1], oh, ol);
        if (rowok[t]) {
          a.XOUT[xpiece(tl[t], ks, 0, lidx[t])] = __builtin_bit_cast(u32x4, oh);
          a.XOUT[xpiece(tl[t], ks, 1, lidx[t])] = __builtin_bit_cast(u32x4, ol);
        }
        if (ztgt) {
          a.zimg[xpiece(zr >> 4, ks, 0, 16 * g + (int)(zr & 15))] = __builtin_bit_cast(u32x4, oh);
          a.zimg[xpiece(zr >> 4, ks, 1, 16 * g + (int)(zr & 15))] = __builtin_bit_cast(u32x4, ol);
        }
        if (!LAST && kp >= 0) {
          a.KXout[xpiece((long)b * (WNK / 16) + (kp >> 4), ks, 0, 16 * g + (kp & 15))] = __builtin_bit_cast(u32x4, oh);
          a.KXout[xpiece((long)b * (WNK / 16) + (kp >> 4), ks, 1, 16 * g + (kp & 15))] = __builtin_bit_cast(u32x4, ol);
        }
      }
    }
  }
  if (wg_tail && !my_tail) idle_chunks(st, seq);       // the tail round of a wave without a unit: stream + barriers only
  st.finish();
  range_check_nan(a.range_flag, range_chk);
}
