// The device body of mfma_filter_kernel_v7<2, FM_IDS, true> (mfma_kernels.hpp includes this file and dispatches to it): the 8-bit, 256-query,
// row-id form of the filter pass on v_mfma_i32_16x16x64_i8.  Everything around the tile is v7's - the 8-bit mirror, the 4-slot LDS-DMA ring of
// 256 rows x 128 B with its granule swizzle and DMA pieces, one barrier and counted waits per K-step, the tile walk, the group rendezvous, the
// pending lists, FilterArgs, the 256 x 256 workgroup tile and the 256 x 64 wavefront tile - only the MFMA shape and what follows from it differ:
//   * profiles/r12_mfma_i8_shape.txt: at equal cycles per MAC the board clocks the 16x16x64 loop 1.13-1.14 x higher than the 32x32x32 loop (row
//     fragments re-read from LDS at this kernel's volume): a quarter of the accumulator registers read and written per instruction, half per MAC.
//   * A wavefront holds 16 row blocks x 4 query blocks of 16 x 16, four accumulator registers each.  A K-step of 128 B is two sub-steps of K = 64;
//     the loop is row-block-outer: the four MFMAs of a row block run back to back on one row fragment.
//   * Row fragment of block i, sub-step s: lane l reads the granule (row 16 i + l % 16, chunk 4 s + l / 16).  The 16 lanes of a phase cover both
//     values of row & 1 and all eight of (row >> 1) & 7: 256 B, conflict-free under swz().  Fragments are single-buffered (16 x 4 registers): block
//     i's registers are reloaded for the next sub-step behind the first MFMA of block i + 1 (block 15's behind block 0's, for the same sub-step),
//     i.e. 15 blocks = 960 matrix cycles ahead of their use, waited for by count (lgkmcnt(14)).
//   * Issue slots of a K-step (128 MFMAs of 16 cycles): 32 fragment reads behind every block's first MFMA; on odd blocks one VMEM operation - its
//     scalar preparation behind the second MFMA, the instruction behind the third: per sub-step four query-fragment loads (blocks 1-7) and four
//     LDS-DMA pieces (blocks 9-15).  Nothing is issued at the end of a step: the second sub-step's query fragments, free only then, are reloaded
//     in the NEXT step's first sub-step (from the previous step's cursor), and the step's closing wait is vmcnt(12) - those four have landed.
//   * A lane's four accumulators of a block are four consecutive rows: the block's start values are one ds_read_b128, and the first sub-step's
//     MFMAs of a tile take it as their C operand (D != C) for all four query blocks - no moves, no initialisation pass.
//   * Epilogue, after the last K-step (no MFMA in flight): per query block four group maxima (row blocks 4 g .. 4 g + 3, eight v_max3_i32 each; the
//     last group reads blocks 14 and 15 out of the accumulator file inside its chain) and their maximum, four compares, one vote and one branch per
//     tile.  The 16 group maxima stay alive to the end of the tile, never across the K loop.  A tile that passes walks, per hit query block, only the
//     groups whose maximum passes (one vote each), and in them the row blocks: block maximum, 4-bit mask, bits.
//     profiles/r17_filter_epilogue.txt: the narrowed walk is worth 1.2-1.8 % of the headline step.  Folding the finished row blocks into the
//     maxima in the issue slots of the tile's last sub-step (two v_max3_i32 behind each MFMA, thresholds read there too) was built and measured
//     beside it: 0.1 %, inside the noise - the step waits for the wavefront with the hit, not for the common path - and is not in this file.
// Query operand: a.qf here is the 16x16x64 fragment-major copy, [b_pad/16][d_pad8/64][64 lanes][16 bytes]: lane l = query l % 16, bytes
// 16 (l / 16) .. + 16 of a K = 64 piece (query_prep8_kernel writes it beside the 32x32x32 copy; launch_filter hands it to this form only).
#pragma once

namespace eps {

struct V7Asm16 {
  template <class A, class F> static __device__ __forceinline__ void v(A& acc, const F& a, const F& b) { asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(a), "a"(b)); }
  template <class A, class F> static __device__ __forceinline__ void a_(A& acc, const F& a, const F& b) { asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc) : "a"(a), "a"(b)); }
  template <class A, class F> static __device__ __forceinline__ void v2(A& d, const F& a, const F& b, const A& c) { asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %3" : "=&v"(d) : "a"(a), "a"(b), "v"(c)); }
  template <class A, class F> static __device__ __forceinline__ void a2(A& d, const F& a, const F& b, const A& c) { asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %3" : "=&a"(d) : "a"(a), "a"(b), "a"(c)); }
};
// max of the 16 accumulators a lane holds of four 16 x 16 blocks (see max16i)
__device__ __forceinline__ int max16i4(const i32x4& p, const i32x4& q, const i32x4& r, const i32x4& t) {
  int d;
  asm("v_max3_i32 %0, %1, %2, %3\n\t"
      "v_max3_i32 %0, %0, %4, %5\n\t"
      "v_max3_i32 %0, %0, %6, %7\n\t"
      "v_max3_i32 %0, %0, %8, %9\n\t"
      "v_max3_i32 %0, %0, %10, %11\n\t"
      "v_max3_i32 %0, %0, %12, %13\n\t"
      "v_max3_i32 %0, %0, %14, %15\n\t"
      "v_max_i32 %0, %0, %16"
      : "=&v"(d)
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]), "v"(t[0]),
        "v"(t[1]), "v"(t[2]), "v"(t[3]));
  return d;
}
// the same with r and t in the accumulator file (row blocks >= V16_VB): read through two temporaries inside the chain, so that the eight values
// are not all copied to arch VGPRs beforehand (32 registers per tile that hipcc makes room for by parking others in the accumulator file)
__device__ __forceinline__ int max16i4_acc(const i32x4& p, const i32x4& q, const i32x4& r, const i32x4& t) {
  int d, x, y;
  asm("v_max3_i32 %0, %3, %4, %5\n\t"
      "v_max3_i32 %0, %0, %6, %7\n\t"
      "v_max3_i32 %0, %0, %8, %9\n\t"
      "v_accvgpr_read_b32 %1, %11\n\t"
      "v_max3_i32 %0, %0, %10, %1\n\t"
      "v_accvgpr_read_b32 %1, %12\n\t"
      "v_accvgpr_read_b32 %2, %13\n\t"
      "v_max3_i32 %0, %0, %1, %2\n\t"
      "v_accvgpr_read_b32 %1, %14\n\t"
      "v_accvgpr_read_b32 %2, %15\n\t"
      "v_max3_i32 %0, %0, %1, %2\n\t"
      "v_accvgpr_read_b32 %1, %16\n\t"
      "v_accvgpr_read_b32 %2, %17\n\t"
      "v_max3_i32 %0, %0, %1, %2\n\t"
      "v_accvgpr_read_b32 %1, %18\n\t"
      "v_max_i32 %0, %0, %1"
      : "=&v"(d), "=&v"(x), "=&v"(y)
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "a"(r[0]), "a"(r[1]), "a"(r[2]), "a"(r[3]), "a"(t[0]),
        "a"(t[1]), "a"(t[2]), "a"(t[3]));
  return d;
}
constexpr int V16_VB = 14;   // row blocks (of 16) whose accumulators live in arch VGPRs: 224 registers, as V7_VI = 7 blocks of 32
#define EPS_DS_READ_B128_V(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))

__device__ __forceinline__ void v7_tile16_ids(const FilterArgs& a) {
  constexpr int NB = 16;                  // 16-row blocks per wavefront
  constexpr int NJ = 4;                   // 16-query blocks per wavefront
  constexpr int TR = 256;                 // rows per tile
  constexpr int VB = V16_VB;
  constexpr int QT = 256;                 // queries per tile
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int ASLOT = TR * 128;
  constexpr int RING = 4;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* base_lds = reinterpret_cast<float*>(lds + RING * ASLOT);  // [2][256]

  const int xcd = blockIdx.x & 7;
  const int local = blockIdx.x >> 3;
  const int per_xcd = gridDim.x >> 3;
  const int QTB = a.tiles_q < per_xcd ? a.tiles_q : per_xcd;
  const int G = per_xcd / QTB;
  const int qslot = local % QTB;
  const int rg = local / QTB;
  if (rg >= G) return;
  const int64_t nj = (a.ntiles - xcd + 7) / 8;
  const int nqt = (a.tiles_q - qslot + QTB - 1) / QTB;
  const int64_t my_rows = nj > rg ? (nj - rg + G - 1) / G : 0;
  const int64_t ntile = my_rows * nqt;
  if (ntile <= 0) return;
  const int ldk = a.d_pad;
  const int KT = ldk / 64;      // even and >= 4

  u32 g_off0;
  auto tile_rt = [&](int ri) { return (int64_t)xcd + 8 * (rg + (int64_t)ri * G); };
  auto tile_qt = [&](int qi) { return qslot + qi * QTB; };
  auto rows_of = [&](int ri) { return a.xh + (a.tile0 + tile_rt(ri)) * TR * (int64_t)ldk; };
  // fragment stream of this wavefront's first 16-query block (halfs); block j follows at + j * jstride, a K = 64 piece is 512 halfs
  const int64_t jstride = (int64_t)(ldk / 32) * 512;
  auto frags_of = [&](int qi) { return a.qf + (int64_t)(tile_qt(qi) * 16 + wave * NJ) * jstride; };
  auto advance = [&](int& ri, int& qi) { if (++qi == nqt) { qi = 0; ++ri; } };
  u32 lane16, lane4;
  const u32 lds_base = (u32)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
  auto issue_base = [&](int ri, int par) {  // start values of row tile ri -> base_lds[par] (64 rows per wavefront)
    const float* pb = a.base_s + (a.tile0 + tile_rt(ri)) * TR + wave * 64;
    const u32 m0v = lds_base + RING * ASLOT + (u32)((par * 256 + wave * 64) * 4);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" : : "v"(lane4), "s"(pb), "s"(m0v) : "memory");
  };
  auto issue_piece = [&](const _Float16* pA, u32 slot_off, int it) {   // pA: first row of the tile, at the K-step to fetch
    const _Float16* sb = pA + (int64_t)it * 32 * ldk;
    const u32 m0v = lds_base + slot_off + (it * 256 + wave * 64) * 16;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(g_off0), "s"(sb), "s"(m0v) : "memory");
  };
  auto prep_piece = [&](const _Float16* pA, u32 slot_off, int it) __attribute__((always_inline)) {
    const _Float16* sb = pA + (int64_t)it * 32 * ldk;
    const u32 m0v = lds_base + slot_off + (it * 256 + wave * 64) * 16;
    asm volatile("s_mov_b32 m0, %1" : "+s"(sb) : "s"(m0v) : "memory");
    return sb;
  };
  auto fire_piece = [&](const _Float16* sb) __attribute__((always_inline)) {
    asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(g_off0), "s"(sb) : "memory");
  };

  i32x4 acc[NB][NJ];
  i32x4 fb[2][2][NJ];   // query fragments of two K-steps: [step parity][sub-step][query block]
  i32x4 fa[NB];         // row fragments of one sub-step
  i32x4 c0[NB];         // a tile's start values, block by block (dead after its first sub-step)
  // Tq: a row passes iff acc >= Tq.  Parked in LDS and read back at each epilogue (as registers they would live across the K loop): [4][64] per
  // wavefront, entry j * 64 + lane = the threshold of query 16 j + lane % 16 of this wavefront
  float* tq_lds = base_lds + 512 + wave * 256;
#pragma unroll
  for (int j = 0; j < NJ; ++j) tq_lds[j * 64 + lane] = a.T[(int64_t)qslot * QT + wave * 64 + j * 16 + (lane & 15)];   // (int32 bits, moved as they are)
  // everything derived from the lane id is re-derived at the top of every tile (see v7: values that live across the tile loop get spilled, and a
  // scratch reload drains the LDS-DMA ring)
  u32 faddr[2], caddr;
  auto lane_values = [&]() __attribute__((always_inline)) {
    u32 ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    lane16 = ln * 16;
    lane4 = ln * 4;
    const u32 td = (u32)wave * 64 + ln, row = td >> 3;
    g_off0 = (row * (u32)ldk + ((td & 7) ^ ((row >> 1) & 7)) * 8) * 2;
#pragma unroll
    for (int s = 0; s < 2; ++s) faddr[s] = lds_base + (u32)swz((int)(ln & 15), s * 4 + (int)(ln >> 4)) * 16;   // + 2048 i: (row >> 1) & 7 is i-free
    caddr = lds_base + RING * ASLOT + (ln >> 4) * 16;   // start values of rows 4 (l / 16) .. + 4 of block 0, parity 0
  };
  lane_values();

  const int64_t a_stride = (int64_t)8 * G * TR * ldk;   // halfs between consecutive row tiles of this workgroup
  int ri_c = 0, qi_c = 0;        // tile t
  int ri_n = 0, qi_n = 0;        // tile t + 1
  advance(ri_n, qi_n);
  const _Float16* A_t = rows_of(0);
  const _Float16* A_n = ntile > 1 ? rows_of(ri_n) : A_t;
  const _Float16* B_t = frags_of(0);
  const _Float16* B_n = (nqt > 1 && ntile > 1) ? frags_of(qi_n) : B_t;
  u32* wcnt = reinterpret_cast<u32*>(lds + RING * ASLOT + 2048 + 4096) + wave * 4;
  u64* wbuf = reinterpret_cast<u64*>(lds + RING * ASLOT + 2048 + 4096 + 64) + wave * V7_CAPW;
  volatile __attribute__((address_space(3))) u32* wcnt_lds = (volatile __attribute__((address_space(3))) u32*)wcnt;
  if (lane == 0) *wcnt = 0;
  auto append = [&](int64_t qq, u32 row) __attribute__((always_inline)) {   // straight to the global list
    const u32 slot_c = atomicAdd(&a.cnt[qq], 1u);
    if (slot_c < (u32)a.cap) a.cand[qq * (int64_t)a.cap + slot_c] = row;
  };
  auto flush = [&]() __attribute__((always_inline)) {
    u32 ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    u32 n = *wcnt_lds;
    n = n < (u32)V7_CAPW ? n : (u32)V7_CAPW;
    for (u32 e = ln; e < n; e += 64) {
      const u64 v = wbuf[e];
      append((int64_t)(v >> 32), (u32)v);
    }
    if (ln == 0) *wcnt_lds = 0;
  };
  const bool rendezvous = a.group_sync && a.tiles_q <= per_xcd;   // (then nqt == 1 for every member of the group)
  u32* gs_ctr = a.group_sync + (xcd * G + rg);
  const int64_t sync_mask = ((int64_t)1 << a.sync_shift) - 1;
  if (rendezvous && wave == 0 && lane == 0) __hip_atomic_fetch_add(gs_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  issue_base(0, 0);
  // prologue = the issue groups of the imaginary steps -3, -2, -1
#pragma unroll
  for (int it = 0; it < 8; ++it) issue_piece(A_t, 0, it);
#pragma unroll
  for (int it = 0; it < 8; ++it) issue_piece(A_t + 64, ASLOT, it);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < NJ; ++j) EPS_GLOAD_B128(fb[0][s][j], lane16, B_t + j * jstride + s * 512, 0);
#pragma unroll
  for (int it = 0; it < 8; ++it) issue_piece(A_t + 128, 2 * ASLOT, it);
  // (step 1's second-sub-step fragments are loaded by step 0's first sub-step, like every step's.  Loading them here as well would leave these
  // loads' registers dead at once: hipcc hands them to the row fragments read below, and the late global load lands on top of those.)
#pragma unroll
  for (int j = 0; j < NJ; ++j) EPS_GLOAD_B128(fb[1][0][j], lane16, B_t + 1024 + j * jstride, 0);
  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // slots 0 and 1 + fragments of step 0
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // blocks 0 .. 14 of the first sub-step (block 15's read goes behind block 0's first MFMA, as in every sub-step)
  EPS_DS_READ_B128(fa[0], faddr[0], 0 * 2048);
  EPS_DS_READ_B128(fa[1], faddr[0], 1 * 2048);
  EPS_DS_READ_B128(fa[2], faddr[0], 2 * 2048);
  EPS_DS_READ_B128(fa[3], faddr[0], 3 * 2048);
  EPS_DS_READ_B128(fa[4], faddr[0], 4 * 2048);
  EPS_DS_READ_B128(fa[5], faddr[0], 5 * 2048);
  EPS_DS_READ_B128(fa[6], faddr[0], 6 * 2048);
  EPS_DS_READ_B128(fa[7], faddr[0], 7 * 2048);
  EPS_DS_READ_B128(fa[8], faddr[0], 8 * 2048);
  EPS_DS_READ_B128(fa[9], faddr[0], 9 * 2048);
  EPS_DS_READ_B128(fa[10], faddr[0], 10 * 2048);
  EPS_DS_READ_B128(fa[11], faddr[0], 11 * 2048);
  EPS_DS_READ_B128(fa[12], faddr[0], 12 * 2048);
  EPS_DS_READ_B128(fa[13], faddr[0], 13 * 2048);
  EPS_DS_READ_B128(fa[14], faddr[0], 14 * 2048);
  // lgkmcnt counts to 15 and the K loop keeps exactly 15 fragment reads in flight: outside the loop they are waited for before anything else
  // that counts there is issued (the rendezvous poll's scalar load, the epilogue's and the head's LDS reads) - with a 16th operation
  // outstanding the counter reads 0 and every wait falls through
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // prefetch cursors, stepped at the end of every K-step (see v7): where this step's LDS-DMA reads (three steps ahead), where its query-fragment
  // loads read (two ahead; and the previous step's cursor, for the fragments that step could not yet reload), and the ring slots
  const _Float16* pA_run = A_t + 3 * 64;
  int akt_run = 3;
  const _Float16* pB_run = B_t + 2 * 1024;
  const _Float16* pBp_run = B_t + 1024;   // (step 0 loads step 1's second-sub-step fragments)
  int bkt_run = 2;
  u32 sA_run = 0, sN_run = ASLOT, sD_run = 3 * ASLOT;
  u32 ad_run = faddr[1];    // where the current sub-step's reads find the NEXT sub-step's fragments
  u32 adh_run = faddr[0];   // ... and block 15's fragment of the current sub-step
  auto step = [&](auto U, auto FIRST) __attribute__((always_inline)) {
    constexpr int rb = decltype(U)::value % 2;
    constexpr bool first = decltype(FIRST)::value;   // first K-step of a tile: its first sub-step takes the start values as C
    const u32 sA = sA_run, sN = sN_run, sD = sD_run;
    const _Float16* pA = pA_run;
    const _Float16* pB = pB_run;
    const _Float16* pBp = pBp_run;
    const _Float16* pA_nx = pA;
    const _Float16* pB_nx = pB;
    int akt_nx = akt_run, bkt_nx = bkt_run;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32 ad = ad_run, adh = adh_run;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const bool has_frag = (i & 1) && i < 8;    // s = 0: the previous step's second-sub-step fragments; s = 1: this step's first-sub-step ones
        const bool has_dma = (i & 1) && i > 8;
        const int jf = i >> 1;                     // (has_frag) query block
        const bool c_in = first && s == 0;
        const _Float16* vsrc = nullptr;
        asm volatile("s_waitcnt lgkmcnt(14)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (c_in) { if (i < VB) V7Asm16::v2(acc[i][0], fa[i], fb[rb][s][0], c0[i]); else V7Asm16::a2(acc[i][0], fa[i], fb[rb][s][0], c0[i]); }
        else { if (i < VB) V7Asm16::v(acc[i][0], fa[i], fb[rb][s][0]); else V7Asm16::a_(acc[i][0], fa[i], fb[rb][s][0]); }
        __builtin_amdgcn_sched_barrier(0);
        switch (i) {
          case 0: EPS_DS_READ_B128(fa[15], adh, 15 * 2048); break;
          case 1: EPS_DS_READ_B128(fa[0], ad, 0 * 2048); break;
          case 2: EPS_DS_READ_B128(fa[1], ad, 1 * 2048); break;
          case 3: EPS_DS_READ_B128(fa[2], ad, 2 * 2048); break;
          case 4: EPS_DS_READ_B128(fa[3], ad, 3 * 2048); break;
          case 5: EPS_DS_READ_B128(fa[4], ad, 4 * 2048); break;
          case 6: EPS_DS_READ_B128(fa[5], ad, 5 * 2048); break;
          case 7: EPS_DS_READ_B128(fa[6], ad, 6 * 2048); break;
          case 8: EPS_DS_READ_B128(fa[7], ad, 7 * 2048); break;
          case 9: EPS_DS_READ_B128(fa[8], ad, 8 * 2048); break;
          case 10: EPS_DS_READ_B128(fa[9], ad, 9 * 2048); break;
          case 11: EPS_DS_READ_B128(fa[10], ad, 10 * 2048); break;
          case 12: EPS_DS_READ_B128(fa[11], ad, 11 * 2048); break;
          case 13: EPS_DS_READ_B128(fa[12], ad, 12 * 2048); break;
          case 14: EPS_DS_READ_B128(fa[13], ad, 13 * 2048); break;
          default: EPS_DS_READ_B128(fa[14], ad, 14 * 2048); break;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c_in) { if (i < VB) V7Asm16::v2(acc[i][1], fa[i], fb[rb][s][1], c0[i]); else V7Asm16::a2(acc[i][1], fa[i], fb[rb][s][1], c0[i]); }
        else { if (i < VB) V7Asm16::v(acc[i][1], fa[i], fb[rb][s][1]); else V7Asm16::a_(acc[i][1], fa[i], fb[rb][s][1]); }
        __builtin_amdgcn_sched_barrier(0);
        if (has_frag) {
          vsrc = (s == 0 ? pBp + 512 : pB) + jf * jstride;
          asm volatile("" : "+s"(vsrc));
        } else if (has_dma) {
          vsrc = prep_piece(pA, sD, s * 4 + ((i - 9) >> 1));
        }
        if (i == NB - 1) {   // the next sub-step's read addresses (s = 1: the next K-step's first sub-step, in the slot after this one)
          u32 adn = faddr[s] + sN;                          // sub-step 1 reads the next step's first fragments, that step's sub-step 0 its second: both in the next slot
          u32 adhn = faddr[s ^ 1] + (s == 0 ? sA : sN);     // block 15 of sub-step 1: this slot; of the next step's sub-step 0: the next slot
          asm volatile("" : "+v"(adn), "+v"(adhn));
          ad_run = adn;
          adh_run = adhn;
        }
        if (s == 1 && i == NB - 2) {   // the next step's cursors
          akt_nx = akt_run + 1;
          pA_nx = pA + 64;
          if (akt_nx == KT) {
            akt_nx = 0;
            pA_nx = A_n;
          }
          bkt_nx = bkt_run + 1;
          pB_nx = pB + 1024;
          if (bkt_nx == KT) {
            bkt_nx = 0;
            pB_nx = B_n;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c_in) { if (i < VB) V7Asm16::v2(acc[i][2], fa[i], fb[rb][s][2], c0[i]); else V7Asm16::a2(acc[i][2], fa[i], fb[rb][s][2], c0[i]); }
        else { if (i < VB) V7Asm16::v(acc[i][2], fa[i], fb[rb][s][2]); else V7Asm16::a_(acc[i][2], fa[i], fb[rb][s][2]); }
        __builtin_amdgcn_sched_barrier(0);
        // (all loads of the loop stay in straight-line code: see v7)
        if (has_frag) {
          if (s == 0) EPS_GLOAD_B128(fb[rb ^ 1][1][jf], lane16, vsrc, 0);
          else EPS_GLOAD_B128(fb[rb][0][jf], lane16, vsrc, 0);
        } else if (has_dma) {
          fire_piece(vsrc);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c_in) { if (i < VB) V7Asm16::v2(acc[i][3], fa[i], fb[rb][s][3], c0[i]); else V7Asm16::a2(acc[i][3], fa[i], fb[rb][s][3], c0[i]); }
        else { if (i < VB) V7Asm16::v(acc[i][3], fa[i], fb[rb][s][3]); else V7Asm16::a_(acc[i][3], fa[i], fb[rb][s][3]); }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    pA_run = pA_nx;
    akt_run = akt_nx;
    pBp_run = pB;
    pB_run = pB_nx;
    bkt_run = bkt_nx;
    sA_run = sN;
    sN_run = (sN + ASLOT) & (RING * ASLOT - 1);
    sD_run = sA;
    // this step's 8 DMA pieces and its last 4 fragment loads may stay in flight; its first 4 (the next step's second sub-step) have landed
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t row0 = (a.tile0 + tile_rt(ri_c)) * TR;
    const int64_t qbase = (int64_t)tile_qt(qi_c) * QT + wave * 64;   // scalar
    lane_values();
    ad_run = faddr[1] + sA_run;
    adh_run = faddr[0] + sA_run;
    if (rendezvous && wave == 0 && (t & sync_mask) == 0) {   // (see v7)
      const u32 want = (u32)QTB * (u32)((t >> a.sync_shift) + 1);
      for (int spin = 0; spin < 1024; ++spin) {
        u32 seen;
        asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(seen) : "s"(gs_ctr) : "memory");
        if (seen >= want) break;
        __builtin_amdgcn_s_sleep(2);
      }
    }
    if (nqt > 1 && t > 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) tq_lds[j * 64 + (lane16 >> 4)] = a.T[(int64_t)tile_qt(qi_c) * QT + wave * 64 + j * 16 + ((lane16 >> 4) & 15)];
    }
    if (t + 1 < ntile) issue_base(ri_n, (int)((t + 1) & 1));
    {
      // the tile's start values: block i's four rows of this lane are one read; its first four MFMAs take them as C.  15 reads, then the 16th
      // once eight have landed (lgkmcnt counts to 15); everything has landed before the K loop, whose counted waits see its own reads alone.
      const u32 ca = caddr + (u32)(t & 1) * 1024;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#define EPS_C0_AT_HEAD(I_)                                                          \
  if ((I_) < VB) EPS_DS_READ_B128_V(c0[(I_)], ca, (I_) * 64);                        \
  else EPS_DS_READ_B128(c0[(I_)], ca, (I_) * 64);
      EPS_C0_AT_HEAD(0) EPS_C0_AT_HEAD(1) EPS_C0_AT_HEAD(2) EPS_C0_AT_HEAD(3) EPS_C0_AT_HEAD(4) EPS_C0_AT_HEAD(5) EPS_C0_AT_HEAD(6) EPS_C0_AT_HEAD(7)
      EPS_C0_AT_HEAD(8) EPS_C0_AT_HEAD(9) EPS_C0_AT_HEAD(10) EPS_C0_AT_HEAD(11) EPS_C0_AT_HEAD(12) EPS_C0_AT_HEAD(13) EPS_C0_AT_HEAD(14)
      asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");
      EPS_C0_AT_HEAD(15)
#undef EPS_C0_AT_HEAD
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    step(std::integral_constant<int, 0>{}, std::true_type{});
    step(std::integral_constant<int, 1>{}, std::false_type{});
    for (int kt = 2; kt < KT; kt += 2) {
      step(std::integral_constant<int, 0>{}, std::false_type{});
      step(std::integral_constant<int, 1>{}, std::false_type{});
    }
    // the asm MFMAs' results are read by VALU code below: hipcc pads nothing after an asm statement
    // (... and the next tile's first fragments, read in the last sub-step, are waited for here: see the prologue)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 7" ::: "memory");
    if (rendezvous && wave == 0 && t + 1 < ntile && ((t + 1) & sync_mask) == 0 && lane16 == 0) __hip_atomic_fetch_add(gs_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    A_t = A_n;
    B_t = B_n;
    ri_c = ri_n;
    qi_c = qi_n;
    {
      const int ri_before = ri_n;
      advance(ri_n, qi_n);
      if (t + 2 < ntile) {
        if (ri_n != ri_before) A_n += a_stride;
        if (nqt > 1) B_n = frags_of(qi_n);
      }
    }
    u32 lne;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lne));
    int Tq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) Tq[j] = __builtin_bit_cast(int, tq_lds[j * 64 + lne]);
    // common path: one running maximum per query block over the tile's 16 row blocks, as v_max3_i32 chains of four blocks each (asm: as C++ the
    // pair maxima are shared with the hit path below and kept alive for it - a hundred registers parked in the accumulator file per tile)
    // The four group maxima of a query block (row blocks 4 g .. 4 g + 3) stay alive until the hit path has used them: 16 registers, from here
    // to the end of the tile only - never across the K loop.
    int mx[NJ], gm[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int g = 0; g < 3; ++g) gm[j][g] = max16i4(acc[4 * g][j], acc[4 * g + 1][j], acc[4 * g + 2][j], acc[4 * g + 3][j]);
      static_assert(VB == NB - 2, "the last group: two blocks in arch VGPRs, two in the accumulator file");
      gm[j][3] = max16i4_acc(acc[12][j], acc[13][j], acc[14][j], acc[15][j]);
      mx[j] = max(max(gm[j][0], gm[j][1]), max(gm[j][2], gm[j][3]));
    }
    const bool h = (mx[0] >= Tq[0]) | (mx[1] >= Tq[1]) | (mx[2] >= Tq[2]) | (mx[3] >= Tq[3]);
    if (__builtin_expect(__any(h), 0)) {
      // (rare) everything the hit path needs is derived behind this opaque copy of the lane id (see v7)
      int lh = (int)lne;
      asm volatile("" : "+v"(lh));
      const int rl = (lh >> 4) * 4;   // the lane's first row within a block
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!__any(mx[j] >= Tq[j])) continue;
        const int64_t qq = qbase + j * 16 + (lh & 15);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          __builtin_amdgcn_sched_barrier(0);
          if (!__any(gm[j][g] >= Tq[j])) continue;   // only the groups of four row blocks that hold a passing row are walked
#pragma unroll
          for (int i = 4 * g; i < 4 * g + 4; ++i) {
            __builtin_amdgcn_sched_barrier(0);   // one block at a time
            const int bm = max(max(acc[i][j][0], acc[i][j][1]), max(acc[i][j][2], acc[i][j][3]));
            if (!__any(bm >= Tq[j])) continue;
            u32 hm = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) hm |= acc[i][j][r] >= Tq[j] ? (1u << r) : 0u;
            if (qq >= a.nq) hm = 0;
            while (hm) {
              const int r = __builtin_ctz(hm);
              hm &= hm - 1;
              const int64_t row64 = row0 + i * 16 + rl + r;
              if (row64 >= a.row_hi) continue;       // (rows beyond the stage's last row: the tile that crosses it)
              const u32 row = (u32)row64;
              const u32 e = atomicAdd(wcnt, 1u);   // LDS: no VMEM counter involved
              if (e < (u32)V7_CAPW) wbuf[e] = ((u64)qq << 32) | row;
              else append(qq, row);
            }
          }
        }
      }
    }
    if (*wcnt_lds >= (u32)(V7_CAPW / 2)) flush();
  }
  flush();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace eps
