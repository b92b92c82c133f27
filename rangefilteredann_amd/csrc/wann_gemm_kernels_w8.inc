// wann_gemm_kernels_w8.inc -- k_gemm_scores for the one-byte shadow rows of a float32 index (WANN_DT = 6; included by
// wann_gemm_kernels_body.inc in place of the float32 / float16 kernel).  Every value of such an index is an integer 0 .. 255: at
// most eight significant bits, so it IS one bfloat16 value -- the row is its own high bf16 term and its low term is zero.  This
// is the bfloat16 unit's kernel (wann_gemm_kernels_bf16.inc) with another point fetch:
//   * the query side, the staged row format (one bf16 row per point, RB = 2 STRIDE + 16 bytes), the two MFMAs per tile and
//     k-step (bh x a_lo, then bh x a_hi), base[], the selection network, the hand-over, the clamped look-ahead row numbers, the
//     LDS size and the two workgroups per CU are that kernel's, line for line: the accumulators hold the float32 kernel's
//     values, because the product it runs first, bl x a_hi, adds only zeros on such a row;
//   * a point arrives as BYTES, a quarter of the float32 row, from the copy the beam searches read (wann_index::d_bytes) or a
//     PrefilterIndex's own (wann_index::d_dense).  The copy is interleaved inside aligned groups of 32 elements (u8_row_position,
//     wann_row_types.h): the 16-byte chunk h of group g holds the four 4-element blocks 2 s + h, s = 0 .. 3, of that group.  Two
//     threads serve a point row, thread h loading chunk h of every group: one 16-byte load a thread and group, four at
//     STRIDE = 128, one at STRIDE <= 32; a lane pair covers 32 contiguous bytes per load instruction.  The row pitch is a
//     multiple of 64 bytes and the padding is zero, so whole groups can always be loaded;
//   * staging widens and un-permutes: a byte b becomes the bf16 pattern of (float)b -- the top half of v_cvt_f32_ubyte0..3's
//     result, exact for 0 .. 255 -- and each block of four goes to its NATURAL element position in the LDS row (8 bytes at
//     64 g + 16 s + 8 h), so the MFMA loop reads the natural-order row the bfloat16 kernel reads.  A STRIDE that is an odd multiple
//     of 16 ends in half a group: its 16 elements are the blocks 0 .. 3, the first two slots of both chunks.
// |p|^2 is the float32 rows' (GemmArgs::pnorm2: k_point_norms of the float32 unit); selection, proof bound and re-rank run in
// the float32 unit on the float32 rows.
// Float8 rows (WANN_DT = 8, wann_gemm_kernels_f8.hip) take this kernel with another widen4_bf16: an OCP E4M3 value has four
// significant bits and an exponent of 2^-9 .. 2^8, so it too IS one bfloat16 value -- v_cvt_pk_f32_fp8 gives the float32, exact
// for every finite pattern in any FP mode (its results are normal numbers), and the top half of that is the bf16.  There the rows
// are the index's own (wann_index::d_points, the same layout), |p|^2 comes from this unit's k_point_norms, and selection, proof
// bound and re-rank run in this unit on the float8 rows: the float32 kernel's scores on the upcast row all the same.
WANN_GNS_BEGIN
// four bytes of a row -> the four bf16 they stand for, in element order
__device__ __forceinline__ uint2 widen4_bf16(uint32_t w) {
#if WANN_DT == 8
  typedef float f8pair_g __attribute__((ext_vector_type(2)));
  const f8pair_g lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  const uint32_t f0 = __float_as_uint(lo.x), f1 = __float_as_uint(lo.y), f2 = __float_as_uint(hi.x), f3 = __float_as_uint(hi.y);
#else
  const uint32_t f0 = __float_as_uint((float)(w & 0xffu)), f1 = __float_as_uint((float)((w >> 8) & 0xffu));
  const uint32_t f2 = __float_as_uint((float)((w >> 16) & 0xffu)), f3 = __float_as_uint((float)(w >> 24));
#endif
  return make_uint2((f0 >> 16) | (f1 & 0xffff0000u), (f2 >> 16) | (f3 & 0xffff0000u));
}

template <int STRIDE>  // row length of the float32 rows (d rounded up to 16): a multiple of 16, <= 128
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
  constexpr int nit = s4 >> 1;  // (the query tile) 128 rows x s4 blocks of four / 256 threads (s4 is even)
  constexpr int G = (STRIDE + 31) / 32;  // 32-element groups of a point row: two threads per row, a 16-byte chunk a thread and group
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
    // The next point block travels HBM -> registers while the MFMA loop of the current one runs, and registers -> bf16 -> LDS
    // after the barrier: thread h of point row tid >> 1 holds chunk h of each of the row's G groups (ix.stride words a row: the
    // byte rows' pitch, whole groups of it always there).  Its row numbers were put in the LDS one step earlier, so no load
    // depends on another load.
    u32x4 pre[G];
    float pre_n = 0.f;
    int pre_rid = 0;
#define WANN_FETCH(C0)                                                                                     \
  {                                                                                                        \
    const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points + (int64_t)rid[tid >> 1] * ix.stride) + 16 * (tid & 1); \
    _Pragma("unroll") for (int x = 0; x < G; x++) pre[x] = *reinterpret_cast<const u32x4 *>(src + 32 * x); \
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
      {
        unsigned char *dst = Ps + (tid >> 1) * RB + 8 * (tid & 1);
#pragma unroll
        for (int x = 0; x < G; x++) {
          const int ns = (32 * x + 32 <= STRIDE) ? 4 : 2;  // (the half group at the end of an odd multiple of 16: blocks 0 .. 3)
#pragma unroll
          for (int s = 0; s < 4; s++)
            if (s < ns) *reinterpret_cast<uint2 *>(dst + 64 * x + 16 * s) = widen4_bf16(pre[x][s]);  // block 2 s + h of group x
        }
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
