// tsim_lw_fast.hip.h - the fused register first pass for the common program shape: ONE compiled component of at most
// 8 outputs (the BASELINE circuits: 5 logical observables in one component), k_sample_lw_fast.
//
// What the generic pass (k_sample_lw_multi) spends outside its Threefry blocks was measured by leaving parts out
// (scripts/lwm_probe.py, profiles/r03/first_pass_breakdown.txt): of 17.4 us per 10^6 shots the five draws are 8.6 -
// the chip's floor for them - and NO memory access matters (f loads, threshold gathers, stores: 0.8-1.0 us each,
// 2.1 together); the other 6.4 us were ~125 vector, ~200 scalar and ~60 scalar-memory instructions per 64 shots:
// 64-bit address arithmetic for every table and key, per-output position loads, divergent while-loops over the
// lane's set bits, select chains over scalar operands.  A scalar instruction costs a SIMD as much issue time as a
// half-rate vector one (4.4 cycles, scripts/microbench/salu_mix.hip).  This kernel removes them instead of tuning them:
//   * everything wave-uniform and loop-invariant is loaded ONCE per block into LDS (rank table, output look-up
//     table, direct-output runs, pattern bases) or once per wave into SGPRs (selection masks, table descriptor);
//   * memory goes through buffer descriptors with 32-bit byte offsets (no 64-bit address arithmetic at all);
//   * the colex rank of the lane's error pattern is a UNIFORM loop over ordinals (trip count = heaviest lane of the
//     wave, no exec masking): per ordinal the lowest set bit of the masked f words, one LDS read of
//     RANK[ordinal][bit position] = C(position inside f_sel, ordinal + 1), precomputed per program;
//   * the n_out sampled bits are placed with ONE look-up LUT[leaf] -> (word 0, word 1) instead of a shift per output;
//   * n_out is a template parameter: the threshold walk is straight-line code.
// Same thresholds, same draws, same hard-row protocol as k_sample_lw_reg / k_sample_lw_multi: bit-identical results
// (tests/test_gpu_steps.py runs every shape through both).
#pragma once
#include "tsim_lw_multi.hip.h"

namespace tsimk {

// header of the fast record in the program image (uint32 words, 64-byte aligned), followed by its tables
enum { LWF_NRUNS = 0, LWF_FLIP0, LWF_FLIP1, LWF_RUNS /* image offset: n_runs x (ctl, mask0, mask1, 0) */,
       LWF_RANK /* image offset: [8][128] words */, LWF_LUT /* image offset: [2^n_out][2] words */, LWF_NOUT, LWF_WORDS = 16 };
#define TSIMK_LWF_MAX_RUNS 32
#define TSIMK_LWF_MAX_NOUT 8

// u < t as integers: see bernoulli_threshold
// PINNED: the statement is volatile, so it keeps its place among the memory instructions round it - reads requested in front of
// a draw stay in front of it, their waits behind it.  Left alone the scheduler puts every draw of k_sample_lw_fast first and
// the threshold reads, each waited for at once, behind them.
// TF_NOP: an s_nop 0 behind every round's add and behind its xor, the two full-rate instructions of the round (none behind the
// half-rate v_alignbit_b32).  The block is one chain of dependent vector instructions, and a wave issues such a chain faster with
// them than without: 35 more instructions per draw and 12 % less time for the block alone (scripts/microbench/threefry_block.hip,
// variant k; profiles/threefry_schedule.txt).  Behind every instruction, or as s_nop 1, they cost time instead.
template <bool PINNED>
__device__ __forceinline__ uint32_t threefry_bits32_lo_at(uint32_t k0, uint32_t k1, uint32_t k0hi, uint32_t lo) {
  // threefry_bits32 for a counter (hi, lo) whose high word is wave-uniform: k0hi = k0 + hi formed on the scalar unit
  const uint32_t k2 = k0 ^ k1 ^ 0x1BD11BDAu;
  uint32_t x0, x1, t;
#define TF_NOP "s_nop 0\n"
#define TF_RN(r) "v_alignbit_b32 %[x1], %[x1], %[x1], " #r "\n v_xor_b32 %[x1], %[x1], %[x0]\n" TF_NOP
#define TF_RA(r) "v_add_u32 %[x0], %[x0], %[x1]\n" TF_NOP TF_RN(r)
#define TF_INJ(kb, i, ka) "s_add_i32 %[t], %[" #kb "], " #i "\n v_add_u32 %[x1], %[t], %[x1]\n v_add3_u32 %[x0], %[x0], %[x1], %[" #ka "]\n"
#define TF_BLOCK                                                                                                           \
  "v_add_u32 %[x1], %[k1], %[lo]\n v_add_u32 %[x0], %[k0hi], %[x1]\n"                                                     \
  TF_RN(19) TF_RA(17) TF_RA(6) TF_RA(26)                                                                                   \
  TF_INJ(k2, 1, k1) TF_RN(15) TF_RA(3) TF_RA(16) TF_RA(8)                                                                  \
  TF_INJ(k0, 2, k2) TF_RN(19) TF_RA(17) TF_RA(6) TF_RA(26)                                                                 \
  TF_INJ(k1, 3, k0) TF_RN(15) TF_RA(3) TF_RA(16) TF_RA(8)                                                                  \
  TF_INJ(k2, 4, k1) TF_RN(19) TF_RA(17) TF_RA(6) TF_RA(26)                                                                 \
  "s_add_i32 %[t], %[k0], 5\n v_add_u32 %[x0], %[k2], %[x0]\n v_add_u32 %[x1], %[t], %[x1]\n v_xor_b32 %[x0], %[x0], %[x1]\n"
#define TF_OPERANDS                                                                                \
  [x0] "=&v"(x0), [x1] "=&v"(x1), [t] "=&s"(t)                                                     \
      : [lo] "v"(lo), [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k0hi] "s"(k0hi)                   \
      : "scc"
  if constexpr (PINNED) asm volatile(TF_BLOCK : TF_OPERANDS);
  else asm(TF_BLOCK : TF_OPERANDS);
#undef TF_OPERANDS
#undef TF_BLOCK
#undef TF_INJ
#undef TF_RA
#undef TF_RN
#undef TF_NOP
  return x0;
}
__device__ __forceinline__ uint32_t threefry_bits32_lo(uint32_t k0, uint32_t k1, uint32_t k0hi, uint32_t lo) {
  return threefry_bits32_lo_at<false>(k0, k1, k0hi, lo);
}

// The threshold walk: node = 2 node + (draw < threshold) per level, the next level's threshold chosen by the bits so far.
// The compare leaves its mask in vcc and v_addc_co_u32 takes it from there as the carry-in of node + node: no bit is made a
// vector (v_cndmask 0, k), none shifted and or-ed in.  Written out because the compiler, given the same sums, selects the
// bits into registers first.  A level's selects by the first bit stand in front of the add that spends vcc; s_nop 1 is the two
// wait states gfx950 wants between a vector instruction's write of a mask and a vector read of it.  t2 = (00, 01, 10, 11).
#define TSIMK_WALK_BIT(d, t) "v_cmp_lt_u32 vcc, %[" #d "], %[" #t "]\n s_nop 1\n"
#define TSIMK_WALK_ADD "v_addc_co_u32 %[n], vcc, %[n], %[n], vcc\n"
__device__ __forceinline__ uint32_t walk1(uint32_t node, uint32_t d0, uint32_t t0) {
  asm(TSIMK_WALK_BIT(d0, t0) TSIMK_WALK_ADD : [n] "+v"(node) : [d0] "v"(d0), [t0] "v"(t0) : "vcc");
  return node;
}
__device__ __forceinline__ uint32_t walk2(uint32_t node, uint32_t d0, uint32_t d1, uint32_t t0, uint32_t t10, uint32_t t11) {
  uint32_t a;
  asm(TSIMK_WALK_BIT(d0, t0) "v_cndmask_b32 %[a], %[t10], %[t11], vcc\n" TSIMK_WALK_ADD
      TSIMK_WALK_BIT(d1, a) TSIMK_WALK_ADD
      : [n] "+v"(node), [a] "=&v"(a) : [d0] "v"(d0), [d1] "v"(d1), [t0] "v"(t0), [t10] "v"(t10), [t11] "v"(t11) : "vcc");
  return node;
}
__device__ __forceinline__ uint32_t walk3(uint32_t node, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t t0, uint32_t t10, uint32_t t11,
                                          uint32_t t200, uint32_t t201, uint32_t t210, uint32_t t211) {
  uint32_t a, p, q;
  asm(TSIMK_WALK_BIT(d0, t0) "v_cndmask_b32 %[a], %[t10], %[t11], vcc\n"
      "v_cndmask_b32 %[p], %[t200], %[t210], vcc\n v_cndmask_b32 %[q], %[t201], %[t211], vcc\n" TSIMK_WALK_ADD
      TSIMK_WALK_BIT(d1, a) "v_cndmask_b32 %[a], %[p], %[q], vcc\n" TSIMK_WALK_ADD
      TSIMK_WALK_BIT(d2, a) TSIMK_WALK_ADD
      : [n] "+v"(node), [a] "=&v"(a), [p] "=&v"(p), [q] "=&v"(q)
      : [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [t0] "v"(t0), [t10] "v"(t10), [t11] "v"(t11), [t200] "v"(t200), [t201] "v"(t201),
        [t210] "v"(t210), [t211] "v"(t211)
      : "vcc");
  return node;
}
#undef TSIMK_WALK_ADD
#undef TSIMK_WALK_BIT

template <int WF32, int NOUT>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(TSIMK_LW_SGPRS))) k_sample_lw_fast(LwMultiArgs M) {
  typedef const __attribute__((address_space(4))) uint8_t *cbytes;
  typedef const __attribute__((address_space(4))) LwStep *cstep;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  constexpr int NPOS = 32 * WF32;                       // f-row bit positions
  constexpr int RSTR = NPOS + 1;                        // a rank row: NPOS entries and a zero (what an exhausted lane reads)
  constexpr int L_RANK = 0;                             // [8][RSTR]
  constexpr int L_LUT = (L_RANK + 8 * RSTR + 1) & ~1;   // [2^NOUT][2], 8-byte aligned
  constexpr int L_RUNS = L_LUT + (2 << NOUT);           // [MAX_RUNS][4]
  constexpr int L_BASES = L_RUNS + 4 * TSIMK_LWF_MAX_RUNS;  // [72]: bases[cnt], cnt <= 64; zeros above wmax
  constexpr int L_WORDS = L_BASES + 72;
  __shared__ uint32_t lds[L_WORDS];
  const int nthr = blockDim.x;  // 1024: every launcher's block size, and what the one-load-per-thread table fill below counts on
  // ---- once per wave: scalars.  What the record headers hold comes with the kernel arguments (LwFastHeader): a block's
  // way to its first draw is the kernel arguments, then the tables and the first f row side by side - not arguments, headers,
  // tables, barrier, f row one after the other
  const uint32_t n_runs = M.fh.n_runs, flip0 = M.fh.flip0, flip1 = M.fh.flip1;
  uint32_t sel[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) sel[w] = w < WF32 ? M.fh.sel[w] : 0u;
  const uint32_t wmax = M.fh.wmax;
  const uint32_t tab_byte = M.fh.tab_byte;
  const uint32_t keybase = M.fh.keybase;
  // the descriptor ends with the tables: a lane whose pattern index means nothing (hard rows) reads zeros, never beyond
  const __amdgpu_buffer_rsrc_t r_tab = __builtin_amdgcn_make_buffer_rsrc((void *)M.tab, 0, M.tab_bytes, 0x00020000);
  cstep steps = (cstep)((cbytes)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(LwMultiArgs, step));
  const uint32_t so_lo = (uint32_t)M.shot_offset, so_hi = (uint32_t)((unsigned long long)M.shot_offset >> 32);

  const uint32_t bps = (uint32_t)M.blocks_per_step;
  const uint32_t total = bps * (uint32_t)M.n_steps;
  uint32_t vb = blockIdx.x;
  if (vb >= total) return;
  uint32_t step = vb / bps, rb = vb - step * bps;
  const uint32_t Bu = (uint32_t)M.B;
  // ---- once per thread: what a row's byte offsets hold of the thread.  The row block's part is wave-uniform: formed on the scalar
  // unit in every trip and handed to the stores as their scalar offset (their descriptors are unbounded; the f load's ends with the
  // batch, and its whole offset stays in the vector operand: the zeros its idle lanes read are the descriptor's range check at work)
  const uint32_t tid = threadIdx.x;
  const uint32_t out_rb = (uint32_t)M.out_rb;
  const uint32_t tid_pad = tid * 8u, tid_rb = tid * out_rb;
  const bool lead_wave = __builtin_amdgcn_readfirstlane((int)tid) == 0;  // the wave that holds thread 0
  // the first row's f words; the NEXT row's are requested at the top of every iteration
  uint32_t n[4] = {0u, 0u, 0u, 0u};
  auto load_f = [&](uint32_t st, uint32_t rbk) {
    // the descriptor ends with the batch: rows beyond it (the last block's idle lanes) read zeros
    const __amdgpu_buffer_rsrc_t r_f = __builtin_amdgcn_make_buffer_rsrc((void *)steps[st].f, 0, Bu * (uint32_t)(4 * WF32), 0x00020000);
    const uint32_t row = rbk * (uint32_t)nthr + threadIdx.x;
    const uint32_t off = row * (uint32_t)(4 * WF32);
    if (TSIMK_LWM_SKIP & 64) { n[0] ^= (row * 0x9E3779B9u) & (row * 0x85EBCA6Bu) & (row * 0xC2B2AE35u) & 0x11111111u; n[1] = 0; return; }
    if constexpr (WF32 == 2) {
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r_f, off, 0, 0);
      n[0] = v.x; n[1] = v.y;
    } else {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r_f, off, 0, 0);
      n[0] = v.x; n[1] = v.y; n[2] = v.z; n[3] = v.w;
    }
  };
  load_f(step, rb);
  // ---- once per block: tables into LDS.  8 x NPOS <= 1024 rank entries, at most 512 look-up words, 128 run words, 8 bases: one
  // load per thread and table, every one requested (behind the f row's) before the first is waited for
  {
    const uint32_t *g = M.img;
    const uint32_t t = threadIdx.x;
    const bool in_rank = t < 8u * (uint32_t)NPOS, in_lut = t < (2u << NOUT), in_runs = t < 4u * n_runs, in_bases = t < 8u;
    const uint32_t rk = t / (uint32_t)NPOS, rp = t % (uint32_t)NPOS;
    uint32_t v_rank = 0u, v_lut = 0u, v_runs = 0u, v_bases = 0u;
    if (in_rank) v_rank = g[M.fh.rank_off + rk * 128u + rp];
    if (in_lut) v_lut = g[M.fh.lut_off + t];
    if (in_runs) v_runs = g[M.fh.runs_off + t];
    if (in_bases) v_bases = g[M.lw_off + LW_BASES_INLINE + t];
    if (in_rank) lds[L_RANK + rk * (uint32_t)RSTR + rp] = v_rank;
    if (t < 8u) lds[L_RANK + t * (uint32_t)RSTR + (uint32_t)NPOS] = 0u;  // what an exhausted lane reads
    if (in_lut) lds[L_LUT + t] = v_lut;
    if (t < 4u * TSIMK_LWF_MAX_RUNS) lds[L_RUNS + t] = v_runs;
    if (t < 72u) lds[L_BASES + t] = v_bases;
    __syncthreads();
  }
  for (;;) {
    cstep S = steps + step;
    const uint32_t row0 = rb * (uint32_t)nthr;  // the row block's first row (< B): scalar
    const uint32_t row = row0 + tid;
    const bool active = tid < Bu - row0;
    uint32_t f[4] = {n[0], n[1], n[2], n[3]};
    uint32_t vb_n = vb + gridDim.x, step_n = step, rb_n = rb + gridDim.x;
    while (rb_n >= bps) { rb_n -= bps; ++step_n; }
    const bool more = vb_n < total;
    if (more) load_f(step_n, rb_n);
    if (rb == 0u) {  // wave-uniform.  Reset the slot's other counter set (nobody else touches it now)
      if (tid <= TSIMK_LW_LISTS) S->ctl_next[32u * tid] = (tid == TSIMK_LW_LISTS) ? 0xFFFFFFFFu : 0u;
    }
    // ---- K14: direct outputs f[idx] ^ flip (sampler.py:140-145): bit-field runs, rotate and mask
    uint32_t o0 = 0u, o1 = 0u;
    for (uint32_t r = 0; r < ((TSIMK_LWM_SKIP & 2) ? 0u : n_runs); ++r) {
      const u32x4 run = *reinterpret_cast<const u32x4 *>(&lds[L_RUNS + 4u * r]);  // same address in every lane: broadcast
      const uint32_t sw = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.x) >> 8;
      uint32_t src = f[0];
#pragma unroll
      for (int w = 1; w < WF32; ++w) src = (sw == (uint32_t)w) ? f[w] : src;
      const uint32_t rot = __builtin_amdgcn_alignbit(src, src, run.x);  // rotate right by ctl & 31
      o0 |= rot & run.y;
      o1 |= rot & run.z;
    }
    o0 ^= flip0;
    o1 ^= flip1;
    // ---- the component: weight test and colex rank of the masked f words (sampler.py:48 without the gather)
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    uint32_t cnt = 0u;
#pragma unroll
    for (int w = 0; w < WF32; ++w) {
      m[w] = f[w] & sel[w];
      cnt += (uint32_t)__builtin_popcount(m[w]);
    }
    // `hard` as a lane predicate and, beside it, as the wave's mask hm: both from the compares' own masks, joined on the scalar unit
    bool hard = cnt > wmax;
    unsigned long long hm = __builtin_amdgcn_ballot_w64(cnt > wmax);
    if (M.has_check && rb == 0u) {  // wave-uniform: one row block in bps holds the normalisation-check row (sampler.py:66-72), always hard
      if (tid == 0u) {
        hard = true;
        S->ctl[32 * TSIMK_LW_LISTS] = row;
      }
      if (lead_wave) hm |= 1ull;
    }
    hm &= __builtin_amdgcn_ballot_w64(tid < Bu - row0);
    hard = hard && active;
    const bool easy = active && !hard;
    uint32_t pat = lds[L_BASES + cnt];
    const uint32_t live = easy ? cnt : 0u;
    // One ordinal: the lowest set bit of the masked words leaves them, its RANK entry joins the index.  An exhausted
    // lane finds position 0xFFFFFFFF (v_ffbl_b32 of 0 is -1, `| 32 w` keeps it) -> the zero at the end of the row.
    auto ordinal = [&](uint32_t k) -> uint32_t {
      uint32_t c[4], t[4];
#pragma unroll
      for (int w = 0; w < WF32; ++w) {
        uint32_t fb;
        asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(m[w]));
        c[w] = w ? (fb | (32u * (uint32_t)w)) : fb;
        t[w] = m[w] & (m[w] - 1u);
      }
      uint32_t p = c[0];
#pragma unroll
      for (int w = 1; w < WF32; ++w) p = p < c[w] ? p : c[w];
      bool lower_zero = m[0] == 0u;
      m[0] = t[0];
#pragma unroll
      for (int w = 1; w < WF32; ++w) {
        const bool z = m[w] == 0u;
        m[w] = lower_zero ? t[w] : m[w];
        lower_zero = lower_zero && z;
      }
      p = p < (uint32_t)NPOS ? p : (uint32_t)NPOS;
      return lds[(uint32_t)L_RANK + k * (uint32_t)RSTR + p];
    };
    if (!(TSIMK_LWM_SKIP & 4)) {
      // The first two ordinals without asking (98 % of the waves hold a lane of weight 2), the rest while a lane
      // needs them.  Lanes that are not `easy` run along: whatever they add up is never used (their table reads stay
      // inside the descriptor).
      const uint32_t r0 = ordinal(0u);
      const uint32_t r1 = ordinal(1u);
      pat += r0 + r1;
      for (uint32_t k = 2u; __builtin_amdgcn_ballot_w64(live > k) != 0ull; ++k) pat += ordinal(k);
    }
    // ---- thresholds of the pattern's prefix tree and the draws (sampler.py:62-79 with the thresholds tabulated)
    const uint32_t thr = tab_byte + (pat << (NOUT + 2));  // byte offset of the pattern's row
    const uint32_t slo = (so_lo + row0) + tid;  // the host launches this kernel only when shot_offset + B stays below the next 2^32
    cptr kp = (cptr)((cbytes)S + __builtin_offsetof(LwStep, keys)) + 2u * keybase;
    // Every output's key is requested before the first draw, and the draws keep their places (PINNED): a level group's
    // threshold reads are under way while its draws run and are waited for behind them.
    uint32_t key0[NOUT], key1[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      key0[o] = kp[2 * o];
      key1[o] = kp[2 * o + 1];
    }
    auto draw = [&](int o) -> uint32_t {
      const uint32_t k0 = key0[o], k1 = key1[o];
      if (TSIMK_LWM_SKIP & 1) return (slo * 0x9E3779B9u + k0 + k1) >> 9;  // diagnostic: no Threefry
      return threefry_bits32_lo_at<true>(k0, k1, k0 + so_hi, slo) >> 9;
    };
    uint32_t node = 1u;
    int i = 0;
    if (TSIMK_LWM_SKIP & 32) {  // diagnostic: thresholds without memory
#pragma unroll
      for (; i < NOUT; ++i) node = 2u * node + (draw(i) < ((thr * 2654435761u + node * 40503u) & 0x7FFFFFu) ? 1u : 0u);
    }
#pragma unroll
    for (; i + 3 <= NOUT; i += 3) {
      const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b32(r_tab, thr + 4u * node, 0, 0);
      // the second level as two words, not a pair: at the root the three reads of levels one and two are one 12-byte read, and a
      // pair in its upper two registers would be copied to an even register first
      const uint32_t t10 = __builtin_amdgcn_raw_buffer_load_b32(r_tab, thr + 8u * node, 0, 0);
      const uint32_t t11 = __builtin_amdgcn_raw_buffer_load_b32(r_tab, thr + 8u * node + 4u, 0, 0);
      const u32x4 t2 = __builtin_amdgcn_raw_buffer_load_b128(r_tab, thr + 16u * node, 0, 0);
      const uint32_t d0 = draw(i), d1 = draw(i + 1), d2 = draw(i + 2);
      node = walk3(node, d0, d1, d2, t0, t10, t11, t2.x, t2.y, t2.z, t2.w);
    }
    if (TSIMK_LWM_SKIP & 32) {
    } else if constexpr (NOUT % 3 == 2) {
      const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b32(r_tab, thr + 4u * node, 0, 0);
      const u32x2 t1 = __builtin_amdgcn_raw_buffer_load_b64(r_tab, thr + 8u * node, 0, 0);
      const uint32_t d0 = draw(i), d1 = draw(i + 1);
      node = walk2(node, d0, d1, t0, t1.x, t1.y);
    } else if constexpr (NOUT % 3 == 1) {
      const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b32(r_tab, thr + 4u * node, 0, 0);
      node = walk1(node, draw(i), t0);
    }
    // ---- place the sampled bits (one look-up: leaf -> the two output words), store the row
    // node = 2^NOUT + leaf: the walk's leading one comes off with the table's constant address (L_LUT >= 2 << NOUT), not with a mask
    static_assert(L_LUT >= (2 << NOUT), "the look-up table's offset must hold the walk's leading one");
    const u32x2 placed = *reinterpret_cast<const u32x2 *>(&lds[(uint32_t)(L_LUT - (2 << NOUT)) + 2u * node]);
    o0 |= placed.x;
    o1 |= placed.y;
    if (TSIMK_LWM_SKIP & 16) n[0] ^= (o0 ^ o1) & 0x10101010u;  // diagnostic: results stay live without stores
    if (easy && !(TSIMK_LWM_SKIP & 16)) {
      uint64_t *out = S->out;
      uint8_t *oc = S->out_compact;
      if (out) {
        const __amdgpu_buffer_rsrc_t r_o = __builtin_amdgcn_make_buffer_rsrc((void *)out, 0, 0xFFFFFFFF, 0x00020000);
        u32x2 v;
        v.x = o0; v.y = o1;
        __builtin_amdgcn_raw_buffer_store_b64(v, r_o, tid_pad, row0 * 8u, 0);
      }
      if (oc) {
        const __amdgpu_buffer_rsrc_t r_c = __builtin_amdgcn_make_buffer_rsrc((void *)oc, 0, 0xFFFFFFFF, 0x00020000);
        // out_rb bytes at row * out_rb (any alignment: the device runs in unaligned-access mode): as few stores as the size allows -
        // 4-byte pieces, then 2, then 1 (20 outputs: a short and a byte instead of three bytes).  The row size is fixed for the
        // launch: a scalar branch picks the size's straight-line code, every piece at a constant offset and a constant shift.
        const uint32_t blk = row0 * out_rb;
        switch (out_rb) {
          case 1:
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)o0, r_c, tid_rb, blk, 0);
            break;
          case 2:
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o0, r_c, tid_rb, blk, 0);
            break;
          case 3:
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o0, r_c, tid_rb, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(o0 >> 16), r_c, tid_rb + 2u, blk, 0);
            break;
          case 4:
            __builtin_amdgcn_raw_buffer_store_b32(o0, r_c, tid_rb, blk, 0);
            break;
          case 5:
            __builtin_amdgcn_raw_buffer_store_b32(o0, r_c, tid_rb, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)o1, r_c, tid_rb + 4u, blk, 0);
            break;
          case 6:
            __builtin_amdgcn_raw_buffer_store_b32(o0, r_c, tid_rb, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o1, r_c, tid_rb + 4u, blk, 0);
            break;
          case 7:
            __builtin_amdgcn_raw_buffer_store_b32(o0, r_c, tid_rb, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o1, r_c, tid_rb + 4u, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(o1 >> 16), r_c, tid_rb + 6u, blk, 0);
            break;
          default:  // 8
            __builtin_amdgcn_raw_buffer_store_b32(o0, r_c, tid_rb, blk, 0);
            __builtin_amdgcn_raw_buffer_store_b32(o1, r_c, tid_rb + 4u, blk, 0);
            break;
        }
      }
    }
    // ---- wave-aggregated append of the hard rows to this batch's lists
    if (hm != 0ull) {
      const int lane = (int)(threadIdx.x & 63u);
      const int leader = __builtin_ctzll(hm);
      uint32_t basei = 0;
      const uint32_t k = rb & (uint32_t)(M.n_lists - 1);  // this row block's sub-list (n_lists is a power of two)
      uint32_t *ctl = S->ctl;
      if (lane == leader) basei = atomicAdd(&ctl[32u * k], (uint32_t)__popcll(hm));
      basei = (uint32_t)__shfl((int)basei, leader, 64);
      if (hard) S->hard_index[(size_t)k * M.list_cap + basei + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull))] = row;
    }
    if (!more) break;
    vb = vb_n;
    step = step_n;
    rb = rb_n;
  }
}

}  // namespace tsimk
