// tsim_rowtab.hip.h - a table of the distinct patterns of bit-packed rows, each with an exact count (tsim_rowtab_*), and
// the lookup decoder that probes such a table.  Rows, xor, test and the keep rule are the row contract of tsim_bitrows.hip.h,
// whose reader these kernels use; a row's pattern (key) is row ^ xor at the key columns, bit i of the key = key column i,
// W = ceil(n_key / 64) words of 64 bits.
//
// Table: open addressing, linear probing, capacity a power of two, slots never freed.  Per slot
//   tags[s]    the word that is compared and swapped, 0 = empty.  n_key <= 63 ("exact"): the key itself | bit 63, so tag
//              equality IS key equality.  Wider keys: a fingerprint (sum of a 64-bit mix per non-zero key word) | bit 63;
//   counts[s]  uint64 rows;   keys[s][W] the key (wide keys only; stored by the lane that won the slot);
//   values[s]  8 bytes the decoder returns (tables loaded from the host only).
// Kernels (one wave owns a tile of 64 rows, row r = lane r, rows staged in LDS as in k_tally; a persistent grid):
//   k_claim   keep mask; every lane's tag; equal tags of the wave merged by a leader loop over ballots (ALU only); the
//             distinct leaders then go on concurrently: first the block's LDS cache (tag -> count, two candidate entries,
//             one 64-bit LDS compare-and-swap); the lane that opens a cache entry, or finds both candidates taken, probes
//             the table: at most `probe` slots, one 64-bit global compare-and-swap on an empty one.  Nobody waits for
//             anybody: a lost swap is looked at (the tag it lost to may be its own) and the probe goes on.  No slot and no
//             empty one within the bound: the rows are counted as overflow.  The winner of a slot stores the key.  The
//             cache is flushed once per block: one global atomic per entry, so a pattern that dominates costs one
//             same-address atomic per block and launch, not one per tile.
//   k_verify  (wide keys; a launch of its own, so every key of k_claim is visible) every kept row's full key against
//             the key stored in the slot its tag leads to: read-only, no atomics on the table.  A mismatch is a
//             fingerprint collision: counted, and tsim_rowtab_read fails.
//   k_decode  the read-only probe on the key columns (the detectors), the full key compared (wide keys), the slot's
//             value XORed with the row's observable columns: kept / kept and wrong / kept and unknown, merged per wave,
//             then per block in LDS, one atomic each per block.
//   k_decode_pred  k_decode that also stores every row's value (0: not kept, unknown) to pred[r], one plain store per lane.
// Keys of a prefix selection (columns 0 .. n_key-1) are read from the staged bytes, in chunks of kChunk bytes for wide
// rows; any other selection is gathered bit by bit from global memory, in key order.
#pragma once
#include "tsim_bitrows.hip.h"

namespace rowtabk {

using namespace bitrows;  // kChunk, kStage, wsync, stage_rows, lds_word, mask_word, cut_pad, row_obs, readlane64
constexpr int kWaves = 4;
constexpr int kCache = 256;          // entries of a block's LDS cache
constexpr uint64_t kUsed = 1ull << 63;

__host__ __device__ inline uint64_t mix64(uint64_t x) {  // (a bijection)
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}
// the contribution of key word w to the fingerprint (zero words add nothing: sparse keys are cheap)
__host__ __device__ inline uint64_t word_hash(uint64_t word, int w) {
  return word ? mix64(word ^ (0x9E3779B97F4A7C15ULL * (uint64_t)(w + 1))) : 0;
}

struct Args {
  const uint8_t *rows;
  long long n, rb;            // rows, row stride in bytes
  int n_cols, used;           // columns; bytes of a row that hold them
  const uint8_t *xr, *test;   // optional rows of `used` bytes (NULL: none)
  int n_key, W;               // key columns, key words
  int direct;                 // the key columns are 0 .. n_key-1
  const int32_t *kcol;        // [n_key] the key columns (device)
  int exact;                  // n_key <= 63: the tag is the key
  int contig, w4;             // stage a tile as one span; dword loads allowed
  int stage_bytes;            // LDS bytes of one wave's staging area
  unsigned long long *tags, *counts, *keys;
  const unsigned long long *values;
  long long cap_mask;         // capacity - 1
  int probe;                  // slots looked at per probe
  unsigned long long *stats;  // [0] kept [1] entries [2] overflow rows [3] collisions
  int obs_lo, obs_hi;         // k_decode: the observable columns
  unsigned long long *dec;    // k_decode: [0] kept [1] wrong [2] unknown
  unsigned long long *pred;   // k_decode_pred: [n] every row's prediction
};

// one wave's tile of rows
struct Tile {
  const uint8_t *src;
  uint8_t *stage;
  int rows, lane;
};

// is lane's row kept?  (the chunks the test mask touches go through LDS)
__device__ __forceinline__ bool tile_kept(const Args &a, const Tile &t) {
  const bool kept = t.lane < t.rows;
  if (!a.test) return kept;
  const int ss = a.contig ? (int)a.rb : kStage;
  const bool a4 = (ss & 3) == 0;
  uint64_t fail = 0;
  for (int b0 = 0; b0 < a.used; b0 += kChunk) {
    const int nb = min(kChunk, a.used - b0);
    const bool any = (t.lane < nb && a.test[b0 + t.lane]) || (t.lane + 64 < nb && a.test[b0 + t.lane + 64]);
    if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
    if (!a.contig) {
      wsync();
      stage_rows(t.stage, t.src, t.rows, b0, nb, a.rb, 0, a.w4, t.lane);
      wsync();
    }
    const uint8_t *p = t.stage + t.lane * ss + (a.contig ? b0 : 0);
    for (int g = 0; g * 8 < nb; ++g) {
      const int b = b0 + g * 8;
      uint64_t tw = mask_word(a.test, b, a.used);
      if (tw == 0) continue;
      tw = cut_pad(tw, b, a.n_cols);
      fail |= (lds_word(p + g * 8, a4) ^ mask_word(a.xr, b, a.used)) & tw;
    }
  }
  return kept && fail == 0;
}

// f(w, word) for the key words w = 0 .. W-1 of lane's row, in order; the whole wave calls it (the staging is the
// wave's); the words of lanes past `rows` are garbage
template <class F>
__device__ __forceinline__ void visit_key(const Args &a, const Tile &t, F f) {
  if (!a.direct) {  // any selection: bit by bit from global memory, in key order
    const uint8_t *row = t.src + (long long)t.lane * a.rb;
    for (int w = 0; w < a.W; ++w) {
      const int nb = min(64, a.n_key - 64 * w);
      uint64_t word = 0;
      if (t.lane < t.rows)
        for (int b = 0; b < nb; ++b) {
          const int c = a.kcol[64 * w + b];
          uint32_t byte = row[c >> 3];
          if (a.xr) byte ^= a.xr[c >> 3];
          word |= (uint64_t)((byte >> (c & 7)) & 1u) << b;
        }
      f(w, word);
    }
    return;
  }
  const int kb = (a.n_key + 7) >> 3;  // the key is a prefix of the row
  const int ss = a.contig ? (int)a.rb : kStage;
  const bool a4 = (ss & 3) == 0;
  for (int b0 = 0; b0 < kb; b0 += kChunk) {
    const int nb = min(kChunk, kb - b0);
    if (!a.contig) {
      wsync();
      stage_rows(t.stage, t.src, t.rows, b0, nb, a.rb, 0, a.w4, t.lane);
      wsync();
    }
    const uint8_t *p = t.stage + t.lane * ss + (a.contig ? b0 : 0);
    for (int g = 0; g * 8 < nb; ++g) {
      const int b = b0 + g * 8;
      uint64_t word = lds_word(p + g * 8, a4) ^ mask_word(a.xr, b, a.used);
      const int past = (b + 8) * 8 - a.n_key;  // (b * 8 < n_key: past < 64)
      if (past > 0) word &= ~0ull >> past;
      f(b >> 3, word);
    }
  }
}

__device__ __forceinline__ uint64_t tile_tag(const Args &a, const Tile &t) {
  uint64_t fp = 0;
  visit_key(a, t, [&](int w, uint64_t word) { fp = a.exact ? word : fp + word_hash(word, w); });
  return fp | kUsed;
}

// the slot of `tag`, or -1.  CLAIM: an empty slot on the way is taken with one compare-and-swap (won: by this lane).
// A tag only ever replaces 0, once: a stale read can only show 0, and the swap then tells the truth.
template <bool CLAIM>
__device__ __forceinline__ long long probe(const Args &a, uint64_t tag, bool &won) {
  long long i = (long long)(mix64(tag) & (uint64_t)a.cap_mask);
  for (int p = 0; p < a.probe; ++p, i = (i + 1) & a.cap_mask) {
    unsigned long long cur = CLAIM ? __hip_atomic_load(&a.tags[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.tags[i];
    if (cur == tag) return i;
    if (cur != 0) continue;
    if (!CLAIM) return -1;
    cur = atomicCAS(&a.tags[i], 0ull, (unsigned long long)tag);
    if (cur == 0) {
      won = true;
      return i;
    }
    if (cur == tag) return i;
  }
  return -1;
}

__device__ __forceinline__ Tile tile_of(const Args &a, long long t, uint8_t *stage, int lane) {
  const long long r0 = t << 6;
  Tile tile{a.rows + r0 * a.rb, stage, (int)min(64LL, a.n - r0), lane};
  if (a.contig) {
    wsync();
    stage_rows(stage, tile.src, tile.rows, 0, a.used, a.rb, 1, a.w4, lane);
    wsync();
  }
  return tile;
}

__global__ void __launch_bounds__(64 * kWaves) k_claim(Args a) {
  extern __shared__ uint64_t lds_raw[];
  unsigned long long *ctag = reinterpret_cast<unsigned long long *>(lds_raw);  // [kCache] the block's cache: tag,
  uint32_t *ccnt = reinterpret_cast<uint32_t *>(ctag + kCache);               // rows,
  int32_t *cslot = reinterpret_cast<int32_t *>(ccnt + kCache);                // the slot its opener found (-1: none)
  uint32_t *stat = reinterpret_cast<uint32_t *>(cslot + kCache);              // kept, new entries, overflow rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *stage = reinterpret_cast<uint8_t *>(stat + 4) + (size_t)wave * a.stage_bytes;
  for (int i = threadIdx.x; i < kCache; i += blockDim.x) {
    ctag[i] = 0;
    ccnt[i] = 0;
    cslot[i] = -1;
  }
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t kept_acc = 0, new_acc = 0;  // wave-uniform
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wave; t < tiles; t += (long long)gridDim.x * kWaves) {
    const Tile tile = tile_of(a, t, stage, lane);
    const bool kept = tile_kept(a, tile);
    const uint64_t keep = __builtin_amdgcn_ballot_w64(kept);
    if (!keep) continue;
    kept_acc += (uint32_t)__popcll(keep);
    const uint64_t tag = tile_tag(a, tile);
    // ---- equal tags of the wave: the first lane of each leads, with the number of its rows
    uint32_t mine = 0;
    uint64_t pending = keep;
    while (pending) {
      const int leader = __builtin_ctzll(pending);
      const uint64_t lt = readlane64(tag, leader);
      const uint64_t same = __builtin_amdgcn_ballot_w64(kept && tag == lt) & pending;
      if (lane == leader) mine = (uint32_t)__popcll(same);
      pending &= ~same;
    }
    // ---- the leaders, concurrently: the block's cache, then the table
    bool won = false;
    long long slot = -1;
    if (mine) {
      const uint64_t h = mix64(tag);
      int e = -1;
      bool opened = false;
#pragma unroll
      for (int way = 0; way < 2 && e < 0; ++way) {
        const int c = (int)(h >> (40 + 10 * way)) & (kCache - 1);
        const unsigned long long old = atomicCAS(&ctag[c], 0ull, (unsigned long long)tag);
        if (old == 0 || old == tag) {
          e = c;
          opened = old == 0;
        }
      }
      if (e >= 0) atomicAdd(&ccnt[e], mine);
      if (e < 0 || opened) {
        slot = probe<true>(a, tag, won);
        if (opened) cslot[e] = (int32_t)slot;
        else if (slot >= 0) atomicAdd(&a.counts[slot], (unsigned long long)mine);
        else atomicAdd(&stat[2], mine);
      }
    }
    const uint64_t winners = __builtin_amdgcn_ballot_w64(won);
    if (winners) {
      new_acc += (uint32_t)__popcll(winners);
      if (!a.exact)
        visit_key(a, tile, [&](int w, uint64_t word) {
          if (won) a.keys[slot * a.W + w] = word;
        });
    }
  }
  if (lane == 0) {
    if (kept_acc) atomicAdd(&stat[0], kept_acc);
    if (new_acc) atomicAdd(&stat[1], new_acc);
  }
  __syncthreads();
  // ---- flush: one global atomic per cache entry
  for (int i = threadIdx.x; i < kCache; i += blockDim.x)
    if (ccnt[i]) {
      if (cslot[i] >= 0) atomicAdd(&a.counts[cslot[i]], (unsigned long long)ccnt[i]);
      else atomicAdd(&stat[2], ccnt[i]);
    }
  __syncthreads();
  if (threadIdx.x < 3 && stat[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

// lane's full key against the key of `slot` (wide keys); the whole wave calls it
__device__ __forceinline__ bool key_differs(const Args &a, const Tile &t, long long slot) {
  bool bad = false;
  visit_key(a, t, [&](int w, uint64_t word) {
    if (slot >= 0 && a.keys[slot * a.W + w] != word) bad = true;
  });
  return bad;
}

__global__ void __launch_bounds__(64 * kWaves) k_verify(Args a) {
  extern __shared__ uint64_t lds_raw[];
  uint32_t *stat = reinterpret_cast<uint32_t *>(lds_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *stage = reinterpret_cast<uint8_t *>(stat + 4) + (size_t)wave * a.stage_bytes;
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t bad_acc = 0;
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wave; t < tiles; t += (long long)gridDim.x * kWaves) {
    const Tile tile = tile_of(a, t, stage, lane);
    const bool kept = tile_kept(a, tile);
    if (!__builtin_amdgcn_ballot_w64(kept)) continue;
    const uint64_t tag = tile_tag(a, tile);
    bool won = false;
    const long long slot = kept ? probe<false>(a, tag, won) : -1;  // (-1: a row that overflowed)
    if (!__builtin_amdgcn_ballot_w64(slot >= 0)) continue;
    bad_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(key_differs(a, tile, slot)));
  }
  if (lane == 0 && bad_acc) atomicAdd(&stat[0], bad_acc);
  __syncthreads();
  if (threadIdx.x == 0 && stat[0]) atomicAdd(&a.stats[3], (unsigned long long)stat[0]);
}

__global__ void __launch_bounds__(64 * kWaves) k_decode(Args a) {
  extern __shared__ uint64_t lds_raw[];
  uint32_t *stat = reinterpret_cast<uint32_t *>(lds_raw);  // kept, wrong, unknown
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *stage = reinterpret_cast<uint8_t *>(stat + 4) + (size_t)wave * a.stage_bytes;
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t kept_acc = 0, wrong_acc = 0, miss_acc = 0;
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wave; t < tiles; t += (long long)gridDim.x * kWaves) {
    const Tile tile = tile_of(a, t, stage, lane);
    const bool kept = tile_kept(a, tile);
    const uint64_t keep = __builtin_amdgcn_ballot_w64(kept);
    if (!keep) continue;
    kept_acc += (uint32_t)__popcll(keep);
    const uint64_t tag = tile_tag(a, tile);
    bool won = false;
    long long slot = kept ? probe<false>(a, tag, won) : -1;
    if (!a.exact && __builtin_amdgcn_ballot_w64(slot >= 0) && key_differs(a, tile, slot)) slot = -1;  // another syndrome's tag
    const uint64_t obs = kept ? row_obs(a, tile.src + (long long)lane * a.rb) : 0;
    const uint64_t pred = slot >= 0 ? a.values[slot] : 0ull;  // an unknown syndrome predicts no flip
    wrong_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && pred != obs));
    miss_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && slot < 0));
  }
  if (lane == 0) {
    if (kept_acc) atomicAdd(&stat[0], kept_acc);
    if (wrong_acc) atomicAdd(&stat[1], wrong_acc);
    if (miss_acc) atomicAdd(&stat[2], miss_acc);
  }
  __syncthreads();
  if (threadIdx.x < 3 && stat[threadIdx.x]) atomicAdd(&a.dec[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

// k_decode with an outlet: the same lookups and counters, and pred[r] = row r's value, 0 for a row that is not kept and for an
// unknown syndrome (the contract of tsim_uf_decode_device's d_pred: every row of the call is written)
__global__ void __launch_bounds__(64 * kWaves) k_decode_pred(Args a) {
  extern __shared__ uint64_t lds_raw[];
  uint32_t *stat = reinterpret_cast<uint32_t *>(lds_raw);  // kept, wrong, unknown
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *stage = reinterpret_cast<uint8_t *>(stat + 4) + (size_t)wave * a.stage_bytes;
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t kept_acc = 0, wrong_acc = 0, miss_acc = 0;
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wave; t < tiles; t += (long long)gridDim.x * kWaves) {
    const Tile tile = tile_of(a, t, stage, lane);
    const bool valid = lane < tile.rows;
    const long long r = (t << 6) + lane;
    const bool kept = tile_kept(a, tile);
    const uint64_t keep = __builtin_amdgcn_ballot_w64(kept);
    if (!keep) {
      if (valid) a.pred[r] = 0ull;
      continue;
    }
    kept_acc += (uint32_t)__popcll(keep);
    const uint64_t tag = tile_tag(a, tile);
    bool won = false;
    long long slot = kept ? probe<false>(a, tag, won) : -1;
    if (!a.exact && __builtin_amdgcn_ballot_w64(slot >= 0) && key_differs(a, tile, slot)) slot = -1;  // another syndrome's tag
    const uint64_t obs = kept ? row_obs(a, tile.src + (long long)lane * a.rb) : 0;
    const uint64_t pred = slot >= 0 ? a.values[slot] : 0ull;  // an unknown syndrome predicts no flip
    if (valid) a.pred[r] = pred;                              // (a row that is not kept has no slot: 0)
    wrong_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && pred != obs));
    miss_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && slot < 0));
  }
  if (lane == 0) {
    if (kept_acc) atomicAdd(&stat[0], kept_acc);
    if (wrong_acc) atomicAdd(&stat[1], wrong_acc);
    if (miss_acc) atomicAdd(&stat[2], miss_acc);
  }
  __syncthreads();
  if (threadIdx.x < 3 && stat[threadIdx.x]) atomicAdd(&a.dec[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

}  // namespace rowtabk
