// wann_gemm_kernels_bytes.inc -- the dense prefilter path for uint8 / int8 rows (WANN_DT = 1 / 2; included by
// wann_gemm_kernels_body.inc inside namespace wann).  Same plan, tiles and hand-over as the float32 kernels, but the scores are
// EXACT: v_mfma_i32_32x32x32_i8 accumulates int32, so a score is the very distance byte_pair (wann_wave.h) returns -- the
// integer sum cast to float -- and there is no error bound, no split into terms and one product instead of three.
//
//   operands   rows are bytes already (zero padded to a multiple of 64); queries are packed by pack_query_word, k_brute's
//              rule, so out-of-range and fractional fp32 queries give the same bytes on both paths.
//   uint8      the MFMA is signed: both operands are biased, x' = x - 128 (x ^ 0x80), over the WHOLE padded row of Kp bytes
//              (padding becomes -128 on both sides).  With S' = sum q'p', sp' = sum p', sq' = sum q' (all over Kp, all exact):
//                sum q p         = S' + 128 sp' + 128 sq' + 16384 Kp      (inner product)
//                sum (q - p)^2   = sum p'^2 + sum q'^2 - 2 S'             (the bias cancels in the difference)
//              int8: the same formulas with bias 0.
//   score      dist = scale S' + term(p) + cq: scale = -2 / -1, term(p) = sum p'^2 / -(128 sp' + 16384 Kp) per point (computed
//              once per index: k_point_terms_b), cq = sum q'^2 / -128 sq' per query (computed by the lane that owns the query).
//              Every term is below 2^26 in magnitude for rows of up to 512 bytes and below 2^28 for rows of up to 2048 bytes
//              (the largest intermediate, sum p'^2 + sum q'^2 <= 130 050 * 2048 < 2^31); int32 could hold rows of 16 512 (uint8)
//              or 65 535 (int8) elements, the dense path takes rows of up to 2048 bytes (kGemmMaxBytes; 512 without
//              WANN_DENSE_LONG_ROWS) and leaves longer ones to the exact scan.
//   hand-over  a lane's four smallest of its 64 scores as 32-bit keys ((dist + off) >> S) << 6 | position: keys order like
//              (dist >> S, position) as plain unsigned numbers, 0xffffffff = no score.  The selection compares integers.
//                rows of up to 512 bytes (k_gemm_scores_b): S = 0, off = 0 (L2: dist >= 0) or 2^25 (inner product: |dist| <=
//                  65 025 * 512 < 2^25); dist + off < 2^26, the key holds the distance itself.
//                rows of 513 .. 2048 bytes (k_gemm_scores_bslab): S = 2, off = 0 (L2) or 2^27 (inner product).  Ranges at 2048
//                  bytes: L2 0 .. 255^2 * 2048 = 133 171 200 (key <= 0x7effffff); uint8 inner product -133 171 200 .. 0 (dist +
//                  off in 1 046 528 .. 2^27); int8 inner product -128 * 128 * 2048 = -2^25 .. 128 * 127 * 2048 = 33 292 288 (dist +
//                  off <= 167 510 016 < 2^28, key <= 0x9fc0003f).  So dist + off >= 0 and every key stays below kNoKeyTest for
//                  every byte pattern of both types.  Such a key holds the distance QUANTISED to multiples of four: what it
//                  gives back, ((key >> 6) << S) - off, is a LOWER BOUND of the distance, at most 3 below it.
//              key_dist / entry_score / select_keys return that lower bound.  It is all k_rerank needs: candidates are re-scored
//              exactly (wave_distances), and a bound only ever claims "no position left out is better than this".
//   ties       everything a block or the selection did not hand over has a key >= the bound's, i.e. a distance >= the bound's
//              distance (its lower bound where S = 2) -- not a larger one.  k_brute orders by (dist, id): an unseen point at the k-th distance might have the
//              smaller id.  k_rerank therefore accepts a top k only when d_k < bound strictly, re-scans blocks whose fourth
//              entry is <= d_k, and sends the rest to k_brute.

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4g __attribute__((ext_vector_type(4)));

constexpr uint32_t kBias4 = WANN_DT == 1 ? 0x80808080u : 0u;
constexpr int kBias = WANN_DT == 1 ? 128 : 0;
constexpr uint32_t kNoKey = 0xffffffffu, kNoKeyTest = 0xf0000000u;  // (the largest real key is below 0xa0000000)
constexpr int kMipsOff = 1 << 25;
constexpr int kLongKeyShift = 2;  // S of rows of more than 512 bytes; their off = kMipsOff << S = 2^27

// the distance a key stands for (KSH = S = 0) or its lower bound (S = 2); the int32 sum cast to float, as byte_pair casts the
// distance: the cast is monotonic, so the float of a lower bound is a lower bound of the float.  S is a template parameter of the
// selection / re-rank kernels (k_rerank / k_rerank_bslab): the kernels of the short rows are the code they were.
template <int METRIC, int KSH>
__device__ __forceinline__ float key_dist(uint32_t key) { return (float)((int)((key >> 6) << KSH) - (METRIC == 1 ? (kMipsOff << KSH) : 0)); }
// what a hand-over entry says about its position's score (kHuge: the block had fewer than four positions)
template <int METRIC, int KSH>
__device__ __forceinline__ float entry_score(float e) {
  const uint32_t key = __float_as_uint(e);
  return key >= kNoKeyTest ? kHuge : key_dist<METRIC, KSH>(key);
}

WANN_GNS_BEGIN
// one wave per row: term(p) of the header, over the biased padded row
__global__ void k_point_terms_b(IndexView ix, int32_t *term) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= ix.n) return;
  const uint32_t *p = reinterpret_cast<const uint32_t *>(ix.points) + row * (int64_t)ix.stride;
  int s1 = 0, s2 = 0;
  for (int i = lane; i < ix.stride; i += 64) {
    const int w = (int)(p[i] ^ kBias4);
    s2 = __builtin_amdgcn_sdot4(w, w, s2, false);
    s1 = __builtin_amdgcn_sdot4(w, 0x01010101, s1, false);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (lane == 0) term[row] = ix.metric == 1 ? -(kBias * s1 + kBias * kBias * 4 * ix.stride) : s2;
}

// x into the sorted m1 <= m2 <= m3 <= m4 (the largest drops out), on unsigned keys: insert4 of the float kernels
__device__ __forceinline__ void insert4u(uint32_t &m1, uint32_t &m2, uint32_t &m3, uint32_t &m4, uint32_t x) {
  asm volatile("v_med3_u32 %0, %1, %2, %0" : "+v"(m4) : "v"(m3), "v"(x));
  asm volatile("v_med3_u32 %0, %1, %2, %0" : "+v"(m3) : "v"(m2), "v"(x));
  asm volatile("v_med3_u32 %0, %1, %2, %0" : "+v"(m2) : "v"(m1), "v"(x));
  asm volatile("v_min_u32 %0, %0, %1" : "+v"(m1) : "v"(x));
}

// k_gemm_scores for byte rows of 64 NCH bytes (NCH = 1 .. 8).  One workgroup (4 waves) per tile = (group, 128 queries,
// kGemmPointChunk positions); per step 128 rows are staged in the LDS as they are (biased for uint8), every wave owns 32
// queries (B operand: 2 NCH x 16 bytes per lane, in registers for the whole tile) and scores them against the 128 rows =
// 4 MFMA tiles x 2 NCH k-steps of 32 bytes.  The next step's rows travel HBM -> registers under the MFMAs and the selection.
// Occupancy assumed: two workgroups per CU (two waves per SIMD, 256 registers each, LDS <= 2 x 36 KiB) up to 256-byte rows,
// one workgroup per CU beyond (LDS 68 KiB at 512 bytes).
template <int NCH>
__global__ __launch_bounds__(256, NCH > 4 ? 1 : 2) void k_gemm_scores_b(GemmArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int SW = 16 * NCH;       // words per row
  constexpr int NK = 2 * NCH;        // MFMA k-steps (32 bytes each)
  constexpr int RB = 64 * NCH + 16;  // bytes per staged row: 16 B so that 8 rows cover all banks
  unsigned char *Ps = smem;                                       // [128][RB]
  int *base = reinterpret_cast<int *>(smem + 128 * RB);           // [128] per staged position: term(p)
  uint32_t *inv = reinterpret_cast<uint32_t *>(base + 128);       // [128] 0 / 0xffffffff: position beyond the window
  int *rid = reinterpret_cast<int *>(inv + 128);                  // [128] point rows of the block being fetched
  const int half = lane >> 5, col = lane & 31;
  const bool mips = ix.metric == 1;
  const bool need_term = !(WANN_DT == 2 && mips);  // (int8 inner product: term(p) = 0)
  const int scale = mips ? -1 : -2;
  const int ntiles = A.plan[P_NTILES];

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const GemmGroup grp = A.groups[A.tile_group[t]];
    const int tl = t - grp.tile0, ch = tl / grp.nqt, q0 = (tl - ch * grp.nqt) << 7;
    const int64_t w = grp.b - grp.a, wlast = w - 1;
    const int64_t p_begin = (int64_t)ch * kGemmPointChunk;
    const int64_t p_end = (p_begin + kGemmPointChunk < w) ? (p_begin + kGemmPointChunk) : w;
    __syncthreads();  // the previous tile is done with the staging area
    const int64_t tlast = p_end - 1;
    if (tid < 128) rid[tid] = window_row(ix, grp.a + min(p_begin + tid, wlast));
    // B operand: query 32 wv + col, bytes 32 s + 16 half + (0..15).  The tile's queries are packed into the staging area
    // (coalesced loads, clamped query rows, dead rows zero), each lane then takes its share and the query's sums.
    for (int idx = tid; idx < 128 * SW; idx += 256) {
      const int r = idx / SW, c = idx - r * SW;
      const bool live = q0 + r < grp.qcount;
      const int64_t qrow = A.gq[grp.qoff + (live ? q0 + r : grp.qcount - 1)];
      const uint32_t pw = __float_as_uint(pack_query_word(A.queries, qrow * ix.d, c, ix.d));
      *reinterpret_cast<uint32_t *>(Ps + r * RB + 4 * c) = live ? pw : 0u;
    }
    __syncthreads();
    i32x4g aq[NK];
    int sq1 = 0, sq2 = 0;
#pragma unroll
    for (int s = 0; s < NK; s++) {
      u32x4 v = *reinterpret_cast<const u32x4 *>(Ps + (32 * wv + col) * RB + 32 * s + 16 * half);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        v[e] ^= kBias4;
        sq2 = __builtin_amdgcn_sdot4((int)v[e], (int)v[e], sq2, false);
        sq1 = __builtin_amdgcn_sdot4((int)v[e], 0x01010101, sq1, false);
      }
      aq[s] = __builtin_bit_cast(i32x4g, v);
    }
    sq1 += __shfl_xor(sq1, 32);
    sq2 += __shfl_xor(sq2, 32);
    const int cq_off = (mips ? -(kBias * sq1) : sq2) + (mips ? kMipsOff : 0);  // cq + the key's offset
    __syncthreads();
    // this lane: query 32 wv + col; register reg of tile j: window position 32 j + (reg & 3) + 8 (reg >> 2) + 4 half
    const int myrow = q0 + 32 * wv + col;
    const bool live = myrow < grp.qcount;
    const int64_t nsteps = (w + 127) >> 7;
    f32x4 *erow = reinterpret_cast<f32x4 *>(A.scores + grp.soff) + ((int64_t)(live ? myrow : q0) * nsteps + (p_begin >> 7)) * 2 + half;
    // fetch: four threads per row (64 B contiguous), 64 rows per pass, two passes; row numbers are clamped to this tile's last
    // position and were put in the LDS one step earlier, so no load depends on another load
    uint4 pre[2 * NCH];
    int pre_t = 0, pre_rid = 0;
#define WANN_FETCHB(C0)                                                                                                        \
  {                                                                                                                            \
    _Pragma("unroll") for (int p = 0; p < 2; p++) {                                                                            \
      const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points + (int64_t)rid[64 * p + (tid >> 2)] * SW) + 16 * (tid & 3); \
      _Pragma("unroll") for (int x = 0; x < NCH; x++) pre[p * NCH + x] = *reinterpret_cast<const uint4 *>(src + 64 * x);       \
    }                                                                                                                          \
    if (tid < 128) {                                                                                                           \
      if (need_term) pre_t = A.pterm[rid[tid]];                                                                                \
      pre_rid = window_row(ix, grp.a + min((C0) + 128 + tid, tlast));                                                            \
    }                                                                                                                          \
  }
    WANN_FETCHB(p_begin)
    i32x16 acc[4];
    for (int64_t c0 = p_begin; c0 < p_end; c0 += 128) {
      // (the barrier that ended the previous step: nobody reads Ps / base / inv / rid any more)
#pragma unroll
      for (int p = 0; p < 2; p++) {
        unsigned char *dst = Ps + (64 * p + (tid >> 2)) * RB + 16 * (tid & 3);
#pragma unroll
        for (int x = 0; x < NCH; x++) {
          uint4 v = pre[p * NCH + x];
          v.x ^= kBias4; v.y ^= kBias4; v.z ^= kBias4; v.w ^= kBias4;
          *reinterpret_cast<uint4 *>(dst + 64 * x) = v;
        }
      }
      if (tid < 128) {
        const bool valid = c0 + tid < p_end;  // positions beyond the window never win
        base[tid] = valid ? pre_t : 0;
        inv[tid] = valid ? 0u : kNoKey;
        rid[tid] = pre_rid;
      }
      __syncthreads();
      WANN_FETCHB(c0 + 128)  // unconditional (row numbers are clamped)
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0;
      const unsigned char *pb = Ps + col * RB + 16 * half;
#pragma unroll
      for (int s = 0; s < NK; s++) {
        i32x4g b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = *reinterpret_cast<const i32x4g *>(pb + j * 32 * RB + 32 * s);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[j], aq[s], acc[j], 0, 0, 0);
      }
      // the four smallest of this lane's 64 keys, sorted; low six bits = 16 j + reg (which position)
      uint32_t m1 = kNoKey, m2 = kNoKey, m3 = kNoKey, m4 = kNoKey;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const i32x4g b4 = *reinterpret_cast<const i32x4g *>(base + 32 * j + 8 * g + 4 * half);
          const u32x4 i4 = *reinterpret_cast<const u32x4 *>(inv + 32 * j + 8 * g + 4 * half);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int dist_off = scale * acc[j][4 * g + r] + b4[r] + cq_off;  // in [0, 2^26)
            const uint32_t x = (((uint32_t)dist_off << 6) | (uint32_t)(16 * j + 4 * g + r)) | i4[r];
            insert4u(m1, m2, m3, m4, x);
          }
        }
      if (live) erow[(c0 - p_begin) >> 6] = __builtin_bit_cast(f32x4, u32x4{m1, m2, m3, m4});
      __syncthreads();  // every wave is done with Ps / base / inv / rid
    }
  }
#undef WANN_FETCHB
}

// Rows of 513 .. 2048 bytes (nine to thirty-two chunks of 64 bytes; quantised embeddings, GIST): a true K-loop with a run-time
// chunk count.  Only the int32 accumulators of the wave's four 32 x 32 tiles live across the slabs of a step; BOTH operands move
// through the LDS in slabs of 256 bytes -- at 2048 bytes the query operand alone would be 256 registers.  The queries arrive
// packed and biased (k_pack_queries_b, once per batch: GemmArgs::qsplit, per query the padded row of 4 stride bytes), so staging
// them is a copy, and the per-query sums are taken once per tile from the packed row.  The unit of work is a (step, slab): stage
// both operands from the registers they were fetched into | barrier | fetch the NEXT unit into registers | the slab's MFMAs |
// barrier.  The last slab runs only the k-steps the row has (rows are multiples of 64 bytes): what the staging areas hold
// beyond them is never read.  Slab of 256 bytes, not 512: 2 x 128 x 272 bytes of operands + 1.5 KiB = 71 168 bytes of LDS and 64
// registers of operands in flight beside the 64 accumulators, so two workgroups share a CU (two waves per SIMD, 256 registers
// each) and one's MFMAs run under the other's staging, barriers and selection; per k-step one ds_read_b128 of the query and four
// of the rows feed four MFMAs.  Tile shape, selection network and hand-over layout are k_gemm_scores_b's; the keys are the
// quantised ones of the header (S = kLongKeyShift).
__global__ void k_pack_queries_b(const float *queries, int64_t nq, int d, int stride, uint32_t *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * stride) return;
  const int64_t q = i / stride;
  out[i] = __float_as_uint(pack_query_word(queries, q * d, (int)(i - q * stride), d)) ^ kBias4;
}

__global__ __launch_bounds__(256, 2) void k_gemm_scores_bslab(GemmArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int W = 256;      // slab width in bytes
  constexpr int S = W / 32;   // MFMA k-steps per slab
  constexpr int RB = W + 16;  // bytes per staged row: 16 B so that 8 rows cover all banks
  constexpr int NX = W / 64;  // 16-byte pieces per thread and half slab
  unsigned char *Ps = smem;                                       // [128][RB] rows of the slab (biased for uint8)
  unsigned char *Qs = smem + 128 * RB;                            // [128][RB] queries of the slab
  int *base = reinterpret_cast<int *>(smem + 2 * 128 * RB);       // [128] per staged position: term(p)
  uint32_t *inv = reinterpret_cast<uint32_t *>(base + 128);       // [128] 0 / 0xffffffff: position beyond the window
  int *rid = reinterpret_cast<int *>(inv + 128);                  // [128] point rows of the step being fetched
  const int half = lane >> 5, col = lane & 31;
  const bool mips = ix.metric == 1;
  const bool need_term = !(WANN_DT == 2 && mips);  // (int8 inner product: term(p) = 0)
  const int scale = mips ? -1 : -2;
  const int ntiles = A.plan[P_NTILES];
  const int kp = ix.stride * 4, nslab = (kp + W - 1) / W;  // padded row in bytes: 576 .. 2048, three to eight slabs
  const unsigned char *qpack = reinterpret_cast<const unsigned char *>(A.qsplit);

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const GemmGroup grp = A.groups[A.tile_group[t]];
    const int tl = t - grp.tile0, ch = tl / grp.nqt, q0 = (tl - ch * grp.nqt) << 7;
    const int64_t w = grp.b - grp.a, wlast = w - 1;
    const int64_t p_begin = (int64_t)ch * kGemmPointChunk;
    const int64_t p_end = (p_begin + kGemmPointChunk < w) ? (p_begin + kGemmPointChunk) : w;
    __syncthreads();  // the previous tile is done with the staging areas and the rows
    const int64_t tlast = p_end - 1;
    if (tid < 128) rid[tid] = window_row(ix, grp.a + min(p_begin + tid, wlast));
    // this thread's two query rows (64 p + tid / 4), packed (rows beyond the group's last query repeat it; their lanes store nothing)
    const unsigned char *qsrc[2];
#pragma unroll
    for (int p = 0; p < 2; p++) qsrc[p] = qpack + (int64_t)A.gq[grp.qoff + min(q0 + 64 * p + (tid >> 2), grp.qcount - 1)] * kp;
    // this lane's query 32 wv + col: its sums over the padded row, once per tile (the two half waves take alternate 16 bytes)
    int sq1 = 0, sq2 = 0;
    {
      const unsigned char *qme = qpack + (int64_t)A.gq[grp.qoff + min(q0 + 32 * wv + col, grp.qcount - 1)] * kp + 16 * half;
      for (int o = 0; o < kp; o += 32) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(qme + o);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          sq2 = __builtin_amdgcn_sdot4((int)v[e], (int)v[e], sq2, false);
          sq1 = __builtin_amdgcn_sdot4((int)v[e], 0x01010101, sq1, false);
        }
      }
    }
    sq1 += __shfl_xor(sq1, 32);
    sq2 += __shfl_xor(sq2, 32);
    const int cq_off = (mips ? -(kBias * sq1) : sq2) + (mips ? (kMipsOff << kLongKeyShift) : 0);  // cq + the key's offset
    __syncthreads();  // the step's rows are in `rid`
    // this lane: query 32 wv + col; register reg of tile j: window position 32 j + (reg & 3) + 8 (reg >> 2) + 4 half
    const int myrow = q0 + 32 * wv + col;
    const bool live = myrow < grp.qcount;
    const int64_t nsteps = (w + 127) >> 7;
    f32x4 *erow = reinterpret_cast<f32x4 *>(A.scores + grp.soff) + ((int64_t)(live ? myrow : q0) * nsteps + (p_begin >> 7)) * 2 + half;
    // fetch pipeline: the next (step, slab) travels to registers during the MFMAs of the current one -- four threads per row (64 B
    // contiguous), 64 rows per pass, two passes, for both operands.  `rid` holds the rows of the step being fetched; it moves on to
    // the next step when a step's LAST slab is staged.  Offsets are clamped into the row: a last, partial slab fetches bytes it
    // never multiplies.  Row numbers are clamped to this tile's last position.
    u32x4 pre[2 * NX], qre[2 * NX];
    int pre_t = 0, pre_rid = 0;
#define WANN_FETCHS(C0, SL, NEWSTEP)                                                                                           \
  {                                                                                                                            \
    _Pragma("unroll") for (int p = 0; p < 2; p++) {                                                                            \
      const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points + (int64_t)rid[64 * p + (tid >> 2)] * ix.stride); \
      _Pragma("unroll") for (int x = 0; x < NX; x++) {                                                                         \
        const int cb = min(W * (SL) + 16 * (tid & 3) + 64 * x, kp - 16);                                                       \
        pre[p * NX + x] = *reinterpret_cast<const u32x4 *>(src + cb);                                                          \
        qre[p * NX + x] = *reinterpret_cast<const u32x4 *>(qsrc[p] + cb);                                                      \
      }                                                                                                                        \
    }                                                                                                                          \
    if ((NEWSTEP) && tid < 128) {                                                                                              \
      if (need_term) pre_t = A.pterm[rid[tid]];                                                                                \
      pre_rid = window_row(ix, grp.a + min((C0) + 128 + tid, tlast));                                                          \
    }                                                                                                                          \
  }
    WANN_FETCHS(p_begin, 0, true)
    i32x16 acc[4];
    for (int64_t c0 = p_begin; c0 < p_end; c0 += 128) {
      for (int sl = 0; sl < nslab; sl++) {
        // (the barrier that ended the previous unit: nobody reads Ps / Qs / base / inv any more)
#pragma unroll
        for (int p = 0; p < 2; p++) {
          unsigned char *dst = Ps + (64 * p + (tid >> 2)) * RB + 16 * (tid & 3);
          unsigned char *qdst = Qs + (64 * p + (tid >> 2)) * RB + 16 * (tid & 3);
#pragma unroll
          for (int x = 0; x < NX; x++) {
            *reinterpret_cast<u32x4 *>(dst + 64 * x) = pre[p * NX + x] ^ kBias4;
            *reinterpret_cast<u32x4 *>(qdst + 64 * x) = qre[p * NX + x];
          }
        }
        if (tid < 128) {
          if (sl == 0) {
            const bool valid = c0 + tid < p_end;  // positions beyond the window never win
            base[tid] = valid ? pre_t : 0;
            inv[tid] = valid ? 0u : kNoKey;
          }
          if (sl == nslab - 1) rid[tid] = pre_rid;
        }
        __syncthreads();
        {  // the next unit: the next slab of this step, or slab 0 of the next step (none after the tile's last unit)
          const bool newstep = sl + 1 == nslab;
          const int nsl = newstep ? 0 : sl + 1;
          if (!newstep || c0 + 128 < p_end) WANN_FETCHS(c0 + 128, nsl, newstep)
        }
        if (sl == 0) {
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][r] = 0;
        }
        const unsigned char *pb = Ps + col * RB + 16 * half;
        const unsigned char *qa = Qs + (32 * wv + col) * RB + 16 * half;
#define WANN_KSTEPS(s)                                                                                                         \
  {                                                                                                                            \
    const i32x4g a = *reinterpret_cast<const i32x4g *>(qa + 32 * (s));                                                         \
    i32x4g b[4];                                                                                                               \
    _Pragma("unroll") for (int j = 0; j < 4; j++) b[j] = *reinterpret_cast<const i32x4g *>(pb + j * 32 * RB + 32 * (s));       \
    _Pragma("unroll") for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[j], a, acc[j], 0, 0, 0);    \
  }
        const int ks = min(S, (kp - W * sl) >> 5);  // k-steps of this slab (workgroup-uniform; even)
        if (ks == S) {
#pragma unroll
          for (int s = 0; s < S; s++) WANN_KSTEPS(s)
        } else {
#pragma unroll 1
          for (int s = 0; s < ks; s++) WANN_KSTEPS(s)
        }
#undef WANN_KSTEPS
        if (sl + 1 < nslab) __syncthreads();  // every wave is done with this slab's operands
      }
      // the four smallest of this lane's 64 keys, sorted; low six bits = 16 j + reg (which position)
      uint32_t m1 = kNoKey, m2 = kNoKey, m3 = kNoKey, m4 = kNoKey;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const i32x4g b4 = *reinterpret_cast<const i32x4g *>(base + 32 * j + 8 * g + 4 * half);
          const u32x4 i4 = *reinterpret_cast<const u32x4 *>(inv + 32 * j + 8 * g + 4 * half);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int dist_off = scale * acc[j][4 * g + r] + b4[r] + cq_off;  // in [0, 2^28)
            const uint32_t x = ((((uint32_t)dist_off >> kLongKeyShift) << 6) | (uint32_t)(16 * j + 4 * g + r)) | i4[r];
            insert4u(m1, m2, m3, m4, x);
          }
        }
      if (live) erow[(c0 - p_begin) >> 6] = __builtin_bit_cast(f32x4, u32x4{m1, m2, m3, m4});
      __syncthreads();  // every wave is done with Ps / Qs / base / inv
    }
#undef WANN_FETCHS
  }
}
WANN_GNS_END

// select_scores on keys: the kSelect smallest keys of the blocks' (three smallest) entries, sorted in lanes 0 .. kSelect-1;
// `cut` / `blk_bound` are the DISTANCES (key_dist with S = KSH: lower bounds for long rows) of the two bounds on everything that was not selected (FLT_MAX = nothing was left out
// that way): an unselected position's distance is >= the bound, possibly equal to it.
template <int METRIC, int KSH, class LOAD>
__device__ __forceinline__ void select_keys(const LOAD &load, int64_t nblk, int &sel_pos, int &sel_cnt, float &cut, float &blk_bound) {
  const int lane = lane_id();
  uint32_t top_s = kNoKey, thr = kNoKey;  // kNoKey = empty slot; thr = lane kSelect-1
  int top_p = 0, filled = 0;
  uint32_t bound = kNoKey;
  for (int64_t b0 = 0; b0 < nblk; b0 += 64) {
    const int64_t blk = b0 + lane;
    const u32x4 e = (blk < nblk) ? __builtin_bit_cast(u32x4, load(blk)) : u32x4{kNoKey, kNoKey, kNoKey, kNoKey};
    bound = min(bound, e[3]);
    if (b0 == 0) {  // the list starts as the kSelect smallest of the first 64 blocks' minima: one bitonic sort across the wave
      uint32_t key = e[0];
      const uint32_t ix6 = e[0] & 63u;
      int pos = (int)((lane >> 1) * 128 + 32 * (ix6 >> 4) + 8 * ((ix6 >> 2) & 3) + 4 * (lane & 1) + (ix6 & 3));
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const uint32_t ok = (uint32_t)__shfl_xor((int)key, j);
          const int op = __shfl_xor(pos, j);
          const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
          const bool swap = take_min ? (ok < key) : (ok > key);  // (equal keys stay where they are)
          key = swap ? ok : key;
          pos = swap ? op : pos;
        }
      top_s = (lane < kSelect) ? key : kNoKey;
      top_p = pos;
      filled = popc64(ballot64(lane < kSelect && key < kNoKeyTest));
      thr = (uint32_t)rdlane((int)top_s, kSelect - 1);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c == 0 && b0 == 0) continue;  // (placed above)
      const uint32_t key = e[c];
      u64 mask = ballot64(key < kNoKeyTest && key < thr);
      while (mask) {
        const int src = ctz64(mask);
        mask &= mask - 1;
        const uint32_t ck = (uint32_t)rdlane((int)key, src);
        if (ck < thr) {  // wave-uniform; thr may have dropped since the ballot
          const int p = popc64(ballot64(top_s <= ck));  // top is sorted: a prefix of the lanes
          // block b0 + src: step (b >> 1), half (b & 1); low bits 16 j + 4 g + r -> position 32 j + 8 g + 4 half + r
          const uint32_t ix6 = ck & 63u;
          const int64_t bb = b0 + src;
          const int cp = (int)((bb >> 1) * 128 + 32 * (ix6 >> 4) + 8 * ((ix6 >> 2) & 3) + 4 * (bb & 1) + (ix6 & 3));
          const uint32_t up_s = (uint32_t)__builtin_amdgcn_update_dpp((int)top_s, (int)top_s, 0x138, 0xf, 0xf, false);
          const int up_p = __builtin_amdgcn_update_dpp(top_p, top_p, 0x138, 0xf, 0xf, false);
          if (lane < kSelect) {
            top_s = (lane == p) ? ck : (lane > p ? up_s : top_s);
            top_p = (lane == p) ? cp : (lane > p ? up_p : top_p);
          }
          filled += filled < kSelect;
          thr = (uint32_t)rdlane((int)top_s, kSelect - 1);
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) bound = min(bound, (uint32_t)__shfl_xor((int)bound, o));
  sel_pos = top_p;
  sel_cnt = filled;
  cut = (filled == kSelect) ? key_dist<METRIC, KSH>(thr) : 3.402823466e+38f;
  blk_bound = (bound >= kNoKeyTest) ? 3.402823466e+38f : key_dist<METRIC, KSH>(bound);
}
