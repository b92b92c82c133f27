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
// (The float8 unit, WANN_DT = 8, includes this file too, for the slab kernel at its end alone: its narrow kernel is
// wann_gemm_kernels_w8.inc's.)
#if WANN_DT == 5
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
#endif  // WANN_DT == 5 (the narrow kernel)

// Bfloat16 rows of 129 .. 2048 elements (opt-in per index: wann_set_dense_long_rows): k_gemm_scores_bfslab, a K-loop over 2 .. 16
// slabs of 128 elements with the work shape, tiles, selection and hand-over of k_gemm_scores_long, and these parts of its own:
//   * the point operand is the row's bytes: a slab of a point is 256 B of bf16, copied HBM -> registers -> LDS as it arrives
//     (no split, no conversion, no VALU work), PB = 272 B a staged row -- the narrow kernel's RB rule, an odd multiple of 16;
//     128 points take 34 KiB where the float32 K-loop stages 66 KiB;
//   * the freed LDS holds a SECOND point buffer: a unit (step, slab) multiplies out of Ps[u & 1] while the next unit is written
//     to Ps[(u + 1) & 1] -- the writes wait for no barrier, and a unit ends with ONE barrier where k_gemm_scores_long has two.
//     (HBM -> LDS directly was not built: global_load_lds writes a wave's 64 x 16 B contiguously, four rows without their pads,
//     so the padded layout the ds_read_b128 of the B operand needs would cost an LDS -> LDS pass; see DESIGN.md 3.5)
//   * the query operand (pre-split by the float32 unit's k_split_queries, qw words a row, [hi | lo] as k_gemm_scores_long stages
//     it) is single-buffered but WAVE-PRIVATE: wave wv multiplies queries 32 wv .. 32 wv + 31 only, so it stages exactly those
//     rows itself, behind its own reads of the previous slab -- LDS operations of one wave complete in order;
//   * a k-step runs two products per tile, bh x a_lo then bh x a_hi: k_gemm_scores_long's order without its bl x a_hi, which
//     on such a row adds only zeros.  The accumulators hold that kernel's values on the upcast rows, bit for bit.
//   * base[] and rid[] are kept per step parity: the next step's values are written while the current step still reads its own.
// Two row lengths, as for float16 rows: a point row is `stride` words = 2 stride elements (padded to 32), the split query and the
// k-steps go by qw = d rounded up to 16 <= 2 stride.  Fetch offsets are clamped into the row / into qw; the last slab runs only
// the k-steps the row has and never reads what the clamped fetches staged beyond them.
// (a namespace of its own: tests/test_bfloat16.py counts the score kernels of dt_bf16 by name)
//
// Float8 rows of 129 .. 2048 elements (WANN_DT = 8; opt-in per index: wann_set_dense_long_float8): k_gemm_scores_f8slab, THIS text
// with another point side -- an E4M3 value is one bfloat16 as well, so everything above holds, and the MFMA loop reads the same
// staged rows.  What differs is how a slab of a point gets there:
//   * it is 128 B of the row, in the interleaved layout of the one-byte rows (u8_row_position): four groups of 32 elements, a
//     group = two 16-byte chunks, chunk h = the blocks of four 2 s + h, s = 0 .. 3.  Two threads serve a point row, as in
//     wann_gemm_kernels_w8.inc: thread h loads chunk h of each of the slab's groups -- four 16-byte loads a thread and unit where
//     the bfloat16 rows take eight, and sixteen prefetch registers instead of thirty-two;
//   * the bytes wait as raw quads while the current unit multiplies and are widened ONCE, where they are staged (widen4_bf16:
//     v_cvt_pk_f32_fp8, top halves -- sixteen calls a thread and unit): all four waves read every staged point, so widening on
//     the read side would do it four times.  Block 2 s + h of group x goes to its NATURAL place, bytes 64 x + 16 s + 8 h of the
//     272-byte row;
//   * a row is `stride` words = 4 stride BYTES = 4 stride elements (padded to 64); qw = d rounded up to 16 <= 4 stride.  A group
//     a k-step reads begins below qw, so all of it lies inside the row: only groups that are never multiplied are fetched from a
//     clamped offset.  Where the last slab ends in half a group (qw an odd multiple of 16: d = 129 .. 144 is qw = 144 in a
//     192-byte row) all four slots of the group are staged all the same -- unlike the narrow kernel's rows (its ns = 2 case) a
//     staged slab row always has room for a whole group, its second half is the row's zero padding, and no k-step reads it.
// (a namespace of its own here too: tests/test_float8.py counts the score kernels of dt_f8 by name)
#if WANN_DT == 8
#define WANN_BF_NS f8_long
#define WANN_BF_KERNEL k_gemm_scores_f8slab
#define WANN_BF_PRE 4  // 16-byte registers of a unit's point fetch: a chunk of each of the slab's four groups
#else
#define WANN_BF_NS bf16_long
#define WANN_BF_KERNEL k_gemm_scores_bfslab
#define WANN_BF_PRE 8  // eight rows, 16 B of each
#endif
namespace WANN_BF_NS {
__global__ __launch_bounds__(256, 2) void WANN_BF_KERNEL(GemmArgs A) {  // (2: a register cap of 256, the unit's; the LDS admits one workgroup)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int W = 128, S = W / 16;
  constexpr int PB = 2 * W + 16;  // bytes per staged point: one bf16 slab row + 16
  constexpr int QB = 4 * W + 16;  // bytes per staged query: hi | lo bf16 + 16
  unsigned char *Ps = smem;                                       // [2][128][PB] points of the current and the next unit
  unsigned char *Qs = smem + 2 * 128 * PB;                        // [128][QB] queries of the slab; rows 32 wv .. + 31 belong to wave wv
  float *base = reinterpret_cast<float *>(Qs + 128 * QB);         // [2][128] per step parity and staged point: |p|^2 / 0
  int *rid = reinterpret_cast<int *>(base + 256);                 // [2][128] per step parity: the step's point rows
  const int half = lane >> 5, col = lane & 31;
  const bool mips = ix.metric == 1;
  const float scale = mips ? -1.f : -2.f;
  const int ntiles = A.plan[P_NTILES];
  const int stride = ix.stride, qw = qv_words(ix), nslab = (qw + W - 1) / W;

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const GemmGroup grp = A.groups[A.tile_group[t]];
    const int tl = t - grp.tile0, ch = tl / grp.nqt, q0 = (tl - ch * grp.nqt) << 7;
    const int64_t w = grp.b - grp.a, wlast = w - 1;
    const int64_t p_begin = (int64_t)ch * kGemmPointChunk;
    const int64_t p_end = (p_begin + kGemmPointChunk < w) ? (p_begin + kGemmPointChunk) : w;
    const int nstep = (int)((p_end - p_begin + 127) >> 7);
    __syncthreads();  // the previous tile is done with the staging areas and the rows
    if (tid < 128) rid[tid] = window_row(ix, grp.a + min(p_begin + tid, wlast));
    // this lane's two query rows, 32 wv + 16 p + lane / 4 (its own wave's), split: qw words, hi pairs then lo pairs (rows beyond
    // the group's last query repeat it; their lanes store nothing)
    const unsigned char *qsrc[2];
#pragma unroll
    for (int p = 0; p < 2; p++)
      qsrc[p] = reinterpret_cast<const unsigned char *>(A.qsplit + (int64_t)A.gq[grp.qoff + min(q0 + 32 * wv + 16 * p + (lane >> 2), grp.qcount - 1)] * qw);
    __syncthreads();  // step 0's rows are in rid[0]
    const int myrow = q0 + 32 * wv + col;
    const bool live = myrow < grp.qcount;
    const int64_t nsteps = (w + 127) >> 7;
    f32x4 *erow = reinterpret_cast<f32x4 *>(A.scores + grp.soff) + ((int64_t)(live ? myrow : q0) * nsteps + (p_begin >> 7)) * 2 + half;
    // A unit's fetch: sixteen threads per point row (256 B contiguous), eight rows per thread; four lanes per query row (64 B
    // contiguous per term).  With a step's first slab come its norms and the NEXT step's rows.
    // (float8 rows: two threads per point row, one row per thread -- chunk tid & 1 of each of the slab's four groups)
    u32x4 pre[WANN_BF_PRE], qre[16];  // qre: pieces 0 .. 3 of a row: hi pairs, 4 .. 7: lo pairs
    float pre_n = 0.f;
    int pre_rid = 0;
#if WANN_DT == 8
#define WANN_BF_FETCH_POINTS(SL)                                                                           \
    {                                                                                                      \
      const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points + (int64_t)rr[tid >> 1] * stride) + 16 * (tid & 1); \
      _Pragma("unroll") for (int x = 0; x < 4; x++) pre[x] = *reinterpret_cast<const u32x4 *>(src + min(W * (SL) + 32 * x, 4 * stride - 32)); \
    }
#else
#define WANN_BF_FETCH_POINTS(SL)                                                                           \
    _Pragma("unroll") for (int i = 0; i < 8; i++) {                                                        \
      const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points + (int64_t)rr[16 * i + (tid >> 4)] * stride); \
      pre[i] = *reinterpret_cast<const u32x4 *>(src + min(2 * W * (SL) + 16 * (tid & 15), 4 * stride - 16)); \
    }
#endif
#define WANN_BF_FETCH(T, SL, NEWSTEP)                                                                      \
  {                                                                                                        \
    const int *rr = rid + 128 * ((T) & 1);                                                                 \
    WANN_BF_FETCH_POINTS(SL)                                                                               \
    _Pragma("unroll") for (int p = 0; p < 2; p++)                                                          \
      _Pragma("unroll") for (int x = 0; x < 8; x++) {                                                      \
        const int cb = 2 * W * (SL) + 16 * (lane & 3) + 64 * (x & 3);                                      \
        qre[p * 8 + x] = *reinterpret_cast<const u32x4 *>(qsrc[p] + (x >> 2) * 2 * qw + min(cb, 2 * qw - 16)); \
      }                                                                                                    \
    if ((NEWSTEP) && tid < 128) {                                                                          \
      if (!mips) pre_n = A.pnorm2[rr[tid]];                                                                \
      pre_rid = window_row(ix, grp.a + min(p_begin + 128 * (int64_t)((T) + 1) + tid, wlast));              \
    }                                                                                                      \
  }
    // ... and its way into the LDS: the points into buffer U & 1, this wave's queries over the slab it has just multiplied
    // (float8 rows: widened here, block 2 s + (tid & 1) of group x to its natural place in the bf16 row)
#if WANN_DT == 8
#define WANN_BF_STAGE_POINTS(U)                                                                            \
    unsigned char *pd = Ps + ((U) & 1) * 128 * PB + (tid >> 1) * PB + 8 * (tid & 1);                       \
    _Pragma("unroll") for (int x = 0; x < 4; x++)                                                          \
      _Pragma("unroll") for (int s = 0; s < 4; s++)                                                        \
        *reinterpret_cast<uint2 *>(pd + 64 * x + 16 * s) = WANN_DT_NS::widen4_bf16(pre[x][s]);
#else
#define WANN_BF_STAGE_POINTS(U)                                                                            \
    unsigned char *pd = Ps + ((U) & 1) * 128 * PB + (tid >> 4) * PB + 16 * (tid & 15);                     \
    _Pragma("unroll") for (int i = 0; i < 8; i++) *reinterpret_cast<u32x4 *>(pd + 16 * i * PB) = pre[i];
#endif
#define WANN_BF_STAGE(U, T, NEWSTEP)                                                                       \
  {                                                                                                        \
    WANN_BF_STAGE_POINTS(U)                                                                                \
    unsigned char *qd = Qs + (32 * wv + (lane >> 2)) * QB + 16 * (lane & 3);                               \
    _Pragma("unroll") for (int p = 0; p < 2; p++)                                                          \
      _Pragma("unroll") for (int x = 0; x < 8; x++)                                                        \
        *reinterpret_cast<u32x4 *>(qd + 16 * p * QB + (x >> 2) * 2 * W + 64 * (x & 3)) = qre[p * 8 + x];   \
    if ((NEWSTEP) && tid < 128) {                                                                          \
      base[128 * ((T) & 1) + tid] = (p_begin + 128 * (int64_t)(T) + tid < p_end) ? (mips ? 0.f : pre_n) : kHuge; /* positions beyond the window never win */ \
      rid[128 * (((T) + 1) & 1) + tid] = pre_rid;                                                          \
    }                                                                                                      \
  }
    WANN_BF_FETCH(0, 0, true)
    WANN_BF_STAGE(0, 0, true)
    __syncthreads();
    f32x16 acc[4];
    int u = 0;  // units of this tile so far: the current one multiplies out of Ps[u & 1]
    for (int st = 0; st < nstep; st++) {
      for (int sl = 0; sl < nslab; sl++, u++) {
        // the next unit: the next slab of this step, or slab 0 of the next step (none after the tile's last unit); its loads
        // are in flight during this unit's MFMAs
        const bool newstep = sl + 1 == nslab;
        const bool more = !newstep || st + 1 < nstep;
        const int nst = newstep ? st + 1 : st, nsl = newstep ? 0 : sl + 1;
        if (more) WANN_BF_FETCH(nst, nsl, newstep)
        if (sl == 0) {
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
        }
        const unsigned char *pb = Ps + (u & 1) * 128 * PB + col * PB + 16 * half;
        const unsigned char *qa = Qs + (32 * wv + col) * QB + 16 * half;
        // two ds_read_b128 of the A operand and four of the B operand per k-step, for eight MFMAs
#define WANN_BF_KSTEP(s)                                                                                   \
  {                                                                                                        \
    const bf16x8 a_hi = *reinterpret_cast<const bf16x8 *>(qa + 32 * (s));                                  \
    const bf16x8 a_lo = *reinterpret_cast<const bf16x8 *>(qa + 2 * W + 32 * (s));                          \
    bf16x8 bh[4];                                                                                          \
    _Pragma("unroll") for (int j = 0; j < 4; j++) bh[j] = *reinterpret_cast<const bf16x8 *>(pb + j * 32 * PB + 32 * (s)); \
    _Pragma("unroll") for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], a_lo, acc[j], 0, 0, 0); \
    _Pragma("unroll") for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], a_hi, acc[j], 0, 0, 0); \
  }
        const int ks = min(S, (qw - W * sl) >> 4);  // k-steps of this slab (workgroup-uniform)
        // (one loop for full and partial slabs, as in k_gemm_scores_hslab: where an unrolled copy and the loop join, the
        // accumulators live twice -- 51 registers spilled under the cap of 256)
#pragma unroll 1
        for (int s = 0; s < ks; s++) WANN_BF_KSTEP(s)
#undef WANN_BF_KSTEP
        if (newstep) {
          // the four smallest of this lane's 64 scores, sorted; low six mantissa bits = 16 j + reg (which position)
          const float *bs = base + 128 * (st & 1);
          float m1 = kHuge, m2 = kHuge, m3 = kHuge, m4 = kHuge;
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
              const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bs + 32 * j + 8 * g + 4 * half);
#pragma unroll
              for (int r = 0; r < 4; r++) {
                const float sc = fmaf(scale, acc[j][4 * g + r], b4[r]);
                const float x = __uint_as_float((__float_as_uint(sc) & ~63u) | (uint32_t)(16 * j + 4 * g + r));
                insert4(m1, m2, m3, m4, x);
              }
            }
          if (live) erow[2 * st] = f32x4{m1, m2, m3, m4};
        }
        if (more) WANN_BF_STAGE(u + 1, nst, newstep)
        __syncthreads();  // the next unit is staged, and every wave is done with this one's point buffer
      }
    }
#undef WANN_BF_FETCH
#undef WANN_BF_STAGE
#undef WANN_BF_FETCH_POINTS
#undef WANN_BF_STAGE_POINTS
  }
}
}  // namespace bf16_long / f8_long
#undef WANN_BF_NS
#undef WANN_BF_KERNEL
#undef WANN_BF_PRE
