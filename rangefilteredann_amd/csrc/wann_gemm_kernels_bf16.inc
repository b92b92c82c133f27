// wann_gemm_kernels_bf16.inc -- k_gemm_scores for bfloat16 rows (WANN_DT = 5; included by wann_gemm_kernels_body.inc in place of
// the float32 / float16 kernel).  The float32 kernel scores q.p as three bf16 products, q1 p1 + q1 p2 + q2 p1, with both operands
// split into a high and a low bf16 term.  A bfloat16 row IS its high term and its low term is zero, so here
//   * a point is staged as ONE bf16 row, copied as it arrives (no split2 on the point side): RB = 2 STRIDE + 16 bytes a point,
//     an odd multiple of 16 whatever STRIDE is, so eight consecutive rows still cover all eight 16-byte bank groups;
//   * a k-step runs two MFMAs per tile, bh x a_lo then bh x a_hi -- the float32 kernel's order after its bl x a_hi, which on
//     such a row adds only zeros: the accumulators hold the float32 kernel's values on the upcast rows, and selection, proof
//     bound and re-rank are the float32 path's unchanged.
// The query side is the float32 kernel's: the tile of 128 float32 queries passes through the staging area (128 x (STRIDE + 4)
// floats) on its way into registers, so the workgroup's LDS stays the float32 kernel's size although the staged points fill
// only half of it -- the launcher, the occupancy (two workgroups per CU) and every tuning figure are unchanged.
WANN_GNS_BEGIN
template <int STRIDE>  // row length of the float32 upcast (d rounded up to 16): a multiple of 16, <= 128
__global__ __launch_bounds__(256, 2) void k_gemm_scores(GemmArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int S = STRIDE / 16;       // MFMA k-steps per product term
  constexpr int QB = 4 * STRIDE + 16;  // bytes per query row of the tile that passes through the staging area
  constexpr int RB = 2 * STRIDE + 16;  // bytes per staged point: one bf16 row, 16 B so that 8 rows cover all banks
  unsigned char *Ps = smem;                                    // [128][RB] (the query tile: [128][QB])
  float *base = reinterpret_cast<float *>(smem + 128 * QB);    // [128] per staged point: |p|^2 / 0
  int *rid = reinterpret_cast<int *>(base + 128);              // [128] point rows of the block being fetched
  constexpr int s4 = STRIDE >> 2;
  constexpr int nit = s4 >> 1;  // 128 rows x s4 blocks of four / 256 threads (s4 is even)
  constexpr int nx = s4 >> 2;   // staging: four threads per point row (32 B contiguous), 64 rows per pass, two passes
  const int half = lane >> 5, col = lane & 31;
  const bool mips = ix.metric == 1;
  const float scale = mips ? -1.f : -2.f;
  const int ntiles = A.plan[P_NTILES];
#ifdef WANN_GEMM_PROF
  unsigned long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long tk0 = __builtin_readcyclecounter();
#endif

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const GemmGroup grp = A.groups[A.tile_group[t]];
    const int tl = t - grp.tile0, ch = tl / grp.nqt, q0 = (tl - ch * grp.nqt) << 7;
    const int64_t w = grp.b - grp.a, wlast = w - 1;
    const int64_t p_begin = (int64_t)ch * kGemmPointChunk;
    const int64_t p_end = (p_begin + kGemmPointChunk < w) ? (p_begin + kGemmPointChunk) : w;
    __syncthreads();  // the previous tile is done with the staging area
    // (row numbers fetched ahead are clamped to THIS tile's last position, as in the float32 kernel)
    const int64_t tlast = p_end - 1;
    if (tid < 128) rid[tid] = window_row(ix, grp.a + min(p_begin + tid, wlast));
    // A operand: row 32 wv + col, columns 16 s + 8 half + (0..7): float32 queries, split into bf16 pairs in registers
    u32x4 ah[S], al[S];
    {
      constexpr int DP = STRIDE + 4;  // 128 x DP floats = 128 x QB bytes
      float *Qs = reinterpret_cast<float *>(Ps);
      const int dlast = ix.d - 1;
#pragma unroll 2
      for (int it = 0; it < nit; it++) {
        const int idx = tid + it * 256;
        const int r = idx / s4, c = (idx - r * s4) * 4;
        const bool live = q0 + r < grp.qcount;
        const float *src = A.queries + (int64_t)A.gq[grp.qoff + (live ? q0 + r : grp.qcount - 1)] * ix.d;
        f32x4 v;
        v[0] = src[min(c + 0, dlast)]; v[1] = src[min(c + 1, dlast)]; v[2] = src[min(c + 2, dlast)]; v[3] = src[min(c + 3, dlast)];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = (live && c + e < ix.d) ? v[e] : 0.f;
        *reinterpret_cast<f32x4 *>(Qs + r * DP + c) = v;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < S; s++) {
        const float *qp = Qs + (32 * wv + col) * DP + 16 * s + 8 * half;
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(qp), v1 = *reinterpret_cast<const f32x4 *>(qp + 4);
        uint32_t h, l;
        split2(v0[0], v0[1], h, l); ah[s][0] = h; al[s][0] = l;
        split2(v0[2], v0[3], h, l); ah[s][1] = h; al[s][1] = l;
        split2(v1[0], v1[1], h, l); ah[s][2] = h; al[s][2] = l;
        split2(v1[2], v1[3], h, l); ah[s][3] = h; al[s][3] = l;
      }
    }
    __syncthreads();
    // The MFMA tile has the points as rows and the queries as columns: this lane holds query 32 wv + col, and register
    // reg of tile j the window position 32 j + (reg & 3) + 8 (reg >> 2) + 4 half: 64 positions of one query per step.
    const int myrow = q0 + 32 * wv + col;
    const bool live = myrow < grp.qcount;
    // this lane's entries: [query][step of the window][half] x 4 floats
    const int64_t nsteps = (w + 127) >> 7;
    f32x4 *erow = reinterpret_cast<f32x4 *>(A.scores + grp.soff) + ((int64_t)(live ? myrow : q0) * nsteps + (p_begin >> 7)) * 2 + half;
    // The next point block travels HBM -> registers while the MFMA loop of the current one runs, and registers -> LDS after
    // the barrier: 8-byte blocks of four bfloat16 (rows are padded to 32 elements: STRIDE elements of a row are always there).
    // Its row numbers were put in the LDS one step earlier, so no load depends on another load.
    uint2 pre[nit];
    float pre_n = 0.f;
    int pre_rid = 0;
#define WANN_FETCH(C0)                                                                                     \
  {                                                                                                        \
    _Pragma("unroll") for (int p = 0; p < 2; p++) {                                                        \
      const unsigned short *src = reinterpret_cast<const unsigned short *>(ix.points + (int64_t)rid[64 * p + (tid >> 2)] * ix.stride) + 4 * (tid & 3); \
      _Pragma("unroll") for (int x = 0; x < nx; x++) pre[p * nx + x] = *reinterpret_cast<const uint2 *>(src + 16 * x); \
    }                                                                                                      \
    if (tid < 128) {                                                                                       \
      if (!mips) pre_n = A.pnorm2[rid[tid]];                                                               \
      pre_rid = window_row(ix, grp.a + min((C0) + 128 + tid, tlast));                                        \
    }                                                                                                      \
  }
    WANN_FETCH(p_begin)
    f32x16 acc[4];
    for (int64_t c0 = p_begin; c0 < p_end; c0 += 128) {
      GPROF_T(t0)
      // (the barrier that ended the previous step: nobody reads Ps / base / rid any more)
#pragma unroll
      for (int p = 0; p < 2; p++) {
        unsigned char *dst = Ps + (64 * p + (tid >> 2)) * RB + 8 * (tid & 3);
#pragma unroll
        for (int x = 0; x < nx; x++) *reinterpret_cast<uint2 *>(dst + 32 * x) = pre[p * nx + x];  // the row is its own bf16 term
      }
      if (tid < 128) {
        base[tid] = (c0 + tid < p_end) ? (mips ? 0.f : pre_n) : kHuge;  // positions beyond the window never win
        rid[tid] = pre_rid;
      }
      GPROF_T(t1)
      __syncthreads();
      GPROF_T(t2)
      WANN_FETCH(c0 + 128)  // unconditional (row numbers are clamped): a conditional fetch would make the compiler wait for it here
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
      // B operand: four ds_read_b128 per k-step feed eight MFMAs
      const unsigned char *pb = Ps + col * RB + 16 * half;
#pragma unroll
      for (int s = 0; s < S; s++) {
        const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[s]), a_lo = __builtin_bit_cast(bf16x8, al[s]);
        bf16x8 bh[4];
#pragma unroll
        for (int j = 0; j < 4; j++) bh[j] = *reinterpret_cast<const bf16x8 *>(pb + j * 32 * RB + 32 * s);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], a_lo, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], a_hi, acc[j], 0, 0, 0);
      }
      GPROF_T(t3)
      // the four smallest of this lane's 64 scores, sorted; low six mantissa bits = 16 j + reg (which position)
      float m1 = kHuge, m2 = kHuge, m3 = kHuge, m4 = kHuge;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const f32x4 b4 = *reinterpret_cast<const f32x4 *>(base + 32 * j + 8 * g + 4 * half);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float sc = fmaf(scale, acc[j][4 * g + r], b4[r]);
            const float x = __uint_as_float((__float_as_uint(sc) & ~63u) | (uint32_t)(16 * j + 4 * g + r));
            if constexpr (STRIDE < 128) insert4(m1, m2, m3, m4, x);
            else insert4_chain(m1, m2, m3, m4, x);  // (as in the float32 kernel)
          }
        }
      if (live) erow[(c0 - p_begin) >> 6] = f32x4{m1, m2, m3, m4};
      GPROF_T(t4)
      __syncthreads();  // every wave is done with Ps / base / rid
      GPROF_T(t5)
      GPROF_ADD(0, t0, t1) GPROF_ADD(1, t1, t2) GPROF_ADD(2, t2, t3) GPROF_ADD(3, t3, t4) GPROF_ADD(4, t4, t5)
    }
  }
#ifdef WANN_GEMM_PROF
  prof_acc[5] = __builtin_readcyclecounter() - tk0;
  if (lane == 0)
    for (int i = 0; i < 8; i++) atomicAdd(A.prof + i, prof_acc[i]);
#endif
#undef WANN_FETCH
}
WANN_GNS_END
