// tsim_shotdata.hip.h - stim's shot-data formats on the device: encoders from bit-packed rows to format bytes and
// decoders from format bytes to bit-packed rows (the host side is csrc/tsim_shotdata.hip).
//
// Rows: row r starts at byte r * rb and holds n columns little-endian (column c = bit c % 8 of byte c / 8); bits past
// column n - 1 in the row's last byte, and bytes past ceil(n / 8), are ignored on input.
//
// Encoders
//   01, b8, ptb64: fixed size.  01: one thread per 8 columns of a row (8 characters, the last one also the '\n').
//     b8: the strided copy k_copy_rows (or the library's k_compact_rows for padded uint64 rows).  ptb64: one wave per
//     (group of 64 shots, 64 columns): lane s loads word w of shot s, 64 ballots transpose the 64 x 64 block, lane b
//     stores the uint64 of column 64 w + b - 512 contiguous bytes per wave.
//   r8, hits, dets: one thread per row, three passes - k_enc_len (the row's byte count from its set bits, an exclusive
//     scan of the block, the block's total), k_scan_sums (one block scans the block totals; the grand total is what the
//     host reads), k_enc_write (the row's bytes at its offset).
// Decoders (the input is a chunk of a file that starts at a row boundary)
//   01, b8, ptb64: fixed size; every byte of a complete row is checked (01) and written where it belongs.
//   r8: byte b advances the stream position by b + (b < 255); the rows are a stream of n + 1 columns, column n being
//     the implicit terminator.  k_sum_bytes + k_scan_sums give every block its start position; k_dec_r8 rescans its
//     block in LDS, so every byte knows its position: it checks that its run stays inside its row, ORs its 1 into the
//     row (vector atomics on the dword that holds the byte), and the terminator of the last row decoded records the
//     bytes consumed.
//   hits, dets: the same scan over newline flags gives every byte its row; the first byte of a token parses it, checks
//     it and ORs its bit in.
// Faults: one uint64 per call, atomicMin of (byte offset << 8 | kind): the first fault in the chunk wins.
// Every address is formed in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdk {

enum Format { F01 = 0, FB8 = 1, FR8 = 2, FPTB64 = 3, FHITS = 4, FDETS = 5 };
enum Fault { kBadChar = 1, kLength = 2, kRange = 3, kPrefix = 4, kRunPast = 5, kTruncated = 6, kSyntax = 7 };

constexpr int kBlock = 256;       // threads per block of the row and byte passes (4 waves)
constexpr int kScanBlock = 1024;  // threads of k_scan_sums

// result block of a decode call (device, int64): [0] scan total, [1] rows decoded, [2] bytes consumed, [3] fault word
struct Res {
  long long total, rows, consumed;
  unsigned long long fault;
};

__device__ __forceinline__ void fault_at(Res *res, long long off, int kind) {
  atomicMin(&res->fault, ((unsigned long long)off << 8) | (unsigned long long)kind);
}

// exclusive scan over the block (blockDim.x a multiple of 64, at most 1024); `total` = the block's sum
__device__ __forceinline__ long long block_excl_scan(long long v, long long &total) {
  __shared__ long long wsum[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int k = 0; k < nw; ++k) {
    const long long s = wsum[k];
    base += k < wid ? s : 0;
    tot += s;
  }
  __syncthreads();  // wsum is reused by the next call
  total = tot;
  return base + x - v;
}

// word w of a row (bits past column n - 1 cleared); w8: the row is 8-byte aligned and rb % 8 == 0
__device__ __forceinline__ uint64_t row_word(const uint8_t *row, int w, int used, int n, bool w8) {
  uint64_t x;
  if (w8) {
    x = reinterpret_cast<const uint64_t *>(row)[w];
  } else {
    x = 0;
    const int b0 = 8 * w, b1 = min(b0 + 8, used);
    for (int b = b0; b < b1; ++b) x |= (uint64_t)row[b] << (8 * (b - b0));
  }
  const int rest = n - 64 * w;
  return rest >= 64 ? x : (rest <= 0 ? 0 : x & ((1ull << rest) - 1));
}

__device__ __forceinline__ int ndigits(unsigned v) {
  int d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}

__device__ __forceinline__ uint8_t *put_uint(uint8_t *p, unsigned v) {
  const int d = ndigits(v);
  for (int k = d - 1; k >= 0; --k) {
    p[k] = (uint8_t)('0' + v % 10);
    v /= 10;
  }
  return p + d;
}

struct EncArgs {
  const uint8_t *rows;
  long long n, rb;  // rows, stride
  int bits, used;   // columns, bytes of a row that hold them
  int w8;           // 8-byte word loads allowed
  int nm, nd;       // dets sections: measurements, detectors (observables: the rest)
  uint8_t *out;
  long long *off;   // per-row offsets within the block (variable-length formats)
  long long *sums;  // per-block totals, scanned in place by k_scan_sums
};

// bytes of one row in a variable-length format
template <int F>
__device__ long long row_len(const EncArgs &a, const uint8_t *row) {
  const int nw = (a.bits + 63) / 64;
  long long len = F == FDETS ? 5 : 0;  // "shot" + '\n'
  int prev = -1, m = 0;
  for (int w = 0; w < nw; ++w) {
    uint64_t x = row_word(row, w, a.used, a.bits, a.w8);
    while (x) {
      const int c = 64 * w + __builtin_ctzll(x);
      x &= x - 1;
      if (F == FR8) {
        len += (c - prev - 1) / 255 + 1;
      } else if (F == FHITS) {
        len += ndigits((unsigned)c) + 1;  // digits and ',' or '\n'
      } else {
        const int k = c < a.nm ? c : (c < a.nm + a.nd ? c - a.nm : c - a.nm - a.nd);
        len += 2 + ndigits((unsigned)k);
      }
      prev = c;
      ++m;
    }
  }
  if (F == FR8) len += (a.bits - prev - 1) / 255 + 1;
  if (F == FHITS && m == 0) len = 1;
  return len;
}

template <int F>
__global__ void __launch_bounds__(kBlock) k_enc_len(EncArgs a) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long len = r < a.n ? row_len<F>(a, a.rows + r * a.rb) : 0;
  long long tot;
  const long long ex = block_excl_scan(len, tot);
  if (r < a.n) a.off[r] = ex;
  if (threadIdx.x == 0) a.sums[blockIdx.x] = tot;
}

// exclusive scan of sums[0 .. n) in place; the grand total goes to *total
__global__ void __launch_bounds__(kScanBlock) k_scan_sums(long long *sums, long long n, long long *total) {
  long long carry = 0;
  for (long long b = 0; b < n; b += kScanBlock) {
    const long long i = b + threadIdx.x;
    const long long v = i < n ? sums[i] : 0;
    long long tot;
    const long long ex = block_excl_scan(v, tot);
    if (i < n) sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

template <int F>
__global__ void __launch_bounds__(kBlock) k_enc_write(EncArgs a) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= a.n) return;
  const uint8_t *row = a.rows + r * a.rb;
  uint8_t *p = a.out + a.sums[blockIdx.x] + a.off[r];
  const int nw = (a.bits + 63) / 64;
  if (F == FDETS) {
    p[0] = 's', p[1] = 'h', p[2] = 'o', p[3] = 't';
    p += 4;
  }
  int prev = -1, m = 0;
  for (int w = 0; w < nw; ++w) {
    uint64_t x = row_word(row, w, a.used, a.bits, a.w8);
    while (x) {
      const int c = 64 * w + __builtin_ctzll(x);
      x &= x - 1;
      if (F == FR8) {
        int gap = c - prev - 1;
        for (; gap >= 255; gap -= 255) *p++ = 255;
        *p++ = (uint8_t)gap;
      } else if (F == FHITS) {
        if (m) *p++ = ',';
        p = put_uint(p, (unsigned)c);
      } else {
        *p++ = ' ';
        if (c < a.nm) {
          *p++ = 'M';
          p = put_uint(p, (unsigned)c);
        } else if (c < a.nm + a.nd) {
          *p++ = 'D';
          p = put_uint(p, (unsigned)(c - a.nm));
        } else {
          *p++ = 'L';
          p = put_uint(p, (unsigned)(c - a.nm - a.nd));
        }
      }
      prev = c;
      ++m;
    }
  }
  if (F == FR8) {
    int gap = a.bits - prev - 1;
    for (; gap >= 255; gap -= 255) *p++ = 255;
    *p = (uint8_t)gap;
  } else {
    *p = '\n';
  }
}

// 01: thread t -> row t / nch, characters 8 j .. 8 j + 7 of it (nch = ceil((n + 1) / 8) groups per row, '\n' included)
__global__ void __launch_bounds__(kBlock) k_enc_01(EncArgs a) {
  const long long line = (long long)a.bits + 1, nch = (line + 7) / 8;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= a.n * nch) return;
  const long long r = t / nch;
  const int j = (int)(t - r * nch);
  const uint8_t *row = a.rows + r * a.rb;
  uint8_t *p = a.out + r * line + 8ll * j;
  const int c0 = 8 * j;
  const unsigned byte = c0 < a.bits ? row[j] : 0u;
  for (int k = 0; k < 8 && c0 + k <= a.bits; ++k) p[k] = c0 + k == a.bits ? '\n' : (uint8_t)('0' + ((byte >> k) & 1));
}

// rows of `used` bytes from stride rb_in to stride rb_out, bits past column n - 1 cleared (b8 encode and decode)
__global__ void __launch_bounds__(kBlock) k_copy_rows(const uint8_t *in, long long rb_in, uint8_t *out, long long rb_out, long long n,
                                                      int used, unsigned tail_mask) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * used) return;
  const long long r = t / used;
  const int j = (int)(t - r * used);
  out[r * rb_out + j] = (uint8_t)(in[r * rb_in + j] & (j == used - 1 ? tail_mask : 255u));
}

// ptb64 encode: wave (g, w) of 64 shots x 64 columns; rows of group g at a.rows + 64 g rb
__global__ void __launch_bounds__(kBlock) k_enc_ptb64(EncArgs a) {
  const int lane = threadIdx.x & 63;
  const long long nw = (a.bits + 63) / 64;
  const long long wave = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const long long groups = a.n / 64;
  if (wave >= groups * nw) return;  // (the whole wave leaves together)
  const long long g = wave / nw;
  const int w = (int)(wave - g * nw);
  const uint64_t x = row_word(a.rows + (64 * g + lane) * a.rb, w, a.used, a.bits, a.w8);
  uint64_t mine = 0;
#pragma unroll 8
  for (int b = 0; b < 64; ++b) {
    const uint64_t m = __ballot((x >> b) & 1);
    if (lane == b) mine = m;
  }
  const long long c = 64ll * w + lane;
  if (c < a.bits) reinterpret_cast<uint64_t *>(a.out)[g * a.bits + c] = mine;
}

struct DecArgs {
  const uint8_t *in;
  long long n_in;
  int final_chunk;
  int bits, used, nm, nd;
  uint8_t *rows;
  long long rb, max_rows;
  long long *sums;
  Res *res;
  long long n_rows, last_len;  // 01 / ptb64: rows (groups) to decode, bytes of the last 01 row (bits + 1 when it is whole)
};

// 01 decode: thread t -> row t / nch, columns 8 j .. 8 j + 7 (nch = max(1, ceil(n / 8))); the last group checks the '\n'
__global__ void __launch_bounds__(kBlock) k_dec_01(DecArgs a) {
  const long long line = (long long)a.bits + 1;
  const long long nch = a.bits > 0 ? (a.bits + 7) / 8 : 1;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= a.n_rows * nch) return;
  const long long r = t / nch;
  const int j = (int)(t - r * nch);
  const long long len = r == a.n_rows - 1 ? a.last_len : line;
  const long long base = r * line;
  const uint8_t *p = a.in + base;
  unsigned byte = 0;
  const int c0 = 8 * j, c1 = min(c0 + 8, a.bits);
  for (int c = c0; c < c1; ++c) {
    if (c >= len) break;
    const uint8_t ch = p[c];
    if (ch == '0' || ch == '1') {
      byte |= (unsigned)(ch - '0') << (c - c0);
    } else {
      fault_at(a.res, base + c, ch == '\n' ? kLength : kBadChar);
      return;
    }
  }
  if (j == nch - 1) {
    if (len == line) {
      const uint8_t ch = p[a.bits];
      if (ch != '\n') fault_at(a.res, base + a.bits, (ch == '0' || ch == '1') ? kLength : kBadChar);
    } else if (len < a.bits) {
      fault_at(a.res, a.n_in, kTruncated);  // the file ends inside the row
    }
  }
  if (c0 < a.bits) a.rows[r * a.rb + j] = (uint8_t)byte;
}

// ptb64 decode: wave (g, w): lane b loads the uint64 of column 64 w + b, 64 ballots give word w of the group's 64 rows
__global__ void __launch_bounds__(kBlock) k_dec_ptb64(DecArgs a) {
  const int lane = threadIdx.x & 63;
  const long long nw = (a.bits + 63) / 64;
  const long long wave = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (wave >= a.n_rows * nw) return;
  const long long g = wave / nw;
  const int w = (int)(wave - g * nw);
  const long long c = 64ll * w + lane;
  uint64_t x = 0;
  if (c < a.bits) {
    const uint8_t *p = a.in + (g * a.bits + c) * 8;
    for (int k = 0; k < 8; ++k) x |= (uint64_t)p[k] << (8 * k);
  }
  uint64_t mine = 0;
#pragma unroll 8
  for (int s = 0; s < 64; ++s) {
    const uint64_t m = __ballot((x >> s) & 1);
    if (lane == s) mine = m;
  }
  uint8_t *row = a.rows + (64 * g + lane) * a.rb;
  const int b1 = min(8 * w + 8, a.used);
  for (int b = 8 * w; b < b1; ++b) row[b] = (uint8_t)(mine >> (8 * (b - 8 * w)));
}

// set column c of row r (rows zeroed beforehand): a dword atomic on the dword that holds the byte
__device__ __forceinline__ void set_bit(const DecArgs &a, long long r, int c) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(a.rows + r * a.rb + (c >> 3));
  unsigned *word = reinterpret_cast<unsigned *>(addr & ~(uintptr_t)3);
  atomicOr(word, (1u << (c & 7)) << (8 * (addr & 3)));
}

__device__ __forceinline__ long long r8_adv(uint8_t b) { return (long long)b + (b < 255 ? 1 : 0); }

// per-block sums of a per-byte value: r8 advances, or newline flags (hits, dets)
template <int F>
__global__ void __launch_bounds__(kBlock) k_sum_bytes(DecArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  long long v = 0;
  if (i < a.n_in) v = F == FR8 ? r8_adv(a.in[i]) : (a.in[i] == '\n' ? 1 : 0);
  long long tot;
  block_excl_scan(v, tot);
  if (threadIdx.x == 0) a.sums[blockIdx.x] = tot;
}

// rows decoded and bytes consumed from the scan total (one thread)
template <int F>
__global__ void k_dec_rows(DecArgs a) {
  Res *res = a.res;
  const long long total = res->total;
  if (F == FR8) {
    const long long line = (long long)a.bits + 1;
    const long long avail = total / line;
    const long long rows = avail < a.max_rows ? avail : a.max_rows;
    res->rows = rows;
    res->consumed = 0;  // (set by the terminator of row rows - 1)
    if (a.final_chunk && avail <= a.max_rows && total % line != 0) fault_at(res, a.n_in, kTruncated);
  } else {  // hits, dets: newline-terminated rows, the last row of the file may lack its '\n'
    const bool tail = a.final_chunk && a.n_in > 0 && a.in[a.n_in - 1] != '\n';
    const long long avail = total + (tail ? 1 : 0);
    const long long rows = avail < a.max_rows ? avail : a.max_rows;
    res->rows = rows;
    res->consumed = (tail && rows == avail) ? a.n_in : 0;  // (else set by the newline of row rows - 1)
  }
}

__global__ void __launch_bounds__(kBlock) k_dec_r8(DecArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const uint8_t b = i < a.n_in ? a.in[i] : 0;
  long long tot;
  const long long p = a.sums[blockIdx.x] + block_excl_scan(i < a.n_in ? r8_adv(b) : 0, tot);
  if (i >= a.n_in) return;
  const long long line = (long long)a.bits + 1;
  const long long r = p / line, start = r * line;
  const long long end = b == 255 ? p + 255 : p + b;  // last zero of the run, or its 1
  if (end > start + a.bits) {
    fault_at(a.res, i, kRunPast);
    return;
  }
  if (b == 255) return;
  const long long rows = a.res->rows;
  if (r >= rows) return;
  const long long c = end - start;
  if (c < a.bits) {
    set_bit(a, r, (int)c);
  } else if (r == rows - 1) {
    a.res->consumed = i + 1;
  }
}

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// digits from position j on, up to a delimiter (',' / '\n' for hits, ' ' / '\n' for dets) or the chunk's end.
// Returns false (and reports) on a bad character; *incomplete when the token reaches the end of a non-final chunk.
__device__ __forceinline__ bool parse_index(const DecArgs &a, long long j, bool dets, long long &v, long long &stop, bool &incomplete) {
  v = 0;
  incomplete = false;
  long long k = j;
  for (; k < a.n_in; ++k) {
    const uint8_t ch = a.in[k];
    if (ch == '\n' || (dets ? ch == ' ' : ch == ',')) break;
    if (!is_digit(ch)) {
      fault_at(a.res, k, kBadChar);
      return false;
    }
    if (v < (1ll << 40)) v = 10 * v + (ch - '0');
  }
  if (k == a.n_in && !a.final_chunk) incomplete = true;
  stop = k;
  return true;
}

template <int F>
__global__ void __launch_bounds__(kBlock) k_dec_text(DecArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const uint8_t ch = i < a.n_in ? a.in[i] : 0;
  long long tot;
  const long long r = a.sums[blockIdx.x] + block_excl_scan(i < a.n_in && ch == '\n' ? 1 : 0, tot);
  if (i >= a.n_in) return;
  const long long rows = a.res->rows;
  if (ch == '\n') {
    if (r == rows - 1) a.res->consumed = i + 1;
    if (F == FHITS) return;
  }
  // a row that the end of a non-final chunk cuts is left for the next call
  const long long newlines = a.res->total;
  if (!a.final_chunk && r >= newlines) return;
  const uint8_t prev = i > 0 ? a.in[i - 1] : '\n';
  if (F == FHITS) {
    if (ch == ',') {
      if (!is_digit(prev)) fault_at(a.res, i, kSyntax);
      else if (i + 1 == a.n_in) fault_at(a.res, a.n_in, kTruncated);
      else if (!is_digit(a.in[i + 1])) fault_at(a.res, i + 1, a.in[i + 1] == ',' || a.in[i + 1] == '\n' ? kSyntax : kBadChar);
      return;
    }
    if (!is_digit(ch)) {
      fault_at(a.res, i, kBadChar);
      return;
    }
    if (is_digit(prev) && i > 0) return;  // inside a token
    long long v, stop;
    bool inc;
    if (!parse_index(a, i, false, v, stop, inc) || inc) return;
    if (v >= a.bits) {
      fault_at(a.res, i, kRange);
      return;
    }
    if (r < rows) set_bit(a, r, (int)v);
  } else {  // dets
    if (prev == '\n') {  // line start: "shot", then ' ', '\n' or the end of the file
      const char *shot = "shot";
      for (int k = 0; k < 4; ++k) {
        if (i + k == a.n_in) {
          if (a.final_chunk) fault_at(a.res, a.n_in, kTruncated);
          return;
        }
        if (a.in[i + k] != (uint8_t)shot[k]) {
          fault_at(a.res, i + k, kSyntax);
          return;
        }
      }
      if (i + 4 < a.n_in && a.in[i + 4] != ' ' && a.in[i + 4] != '\n') fault_at(a.res, i + 4, kSyntax);
      return;
    }
    if (ch == ' ') {
      if (i + 1 < a.n_in && a.in[i + 1] == '\n') fault_at(a.res, i + 1, kSyntax);  // (a space must precede a token)
      else if (i + 1 == a.n_in && a.final_chunk) fault_at(a.res, a.n_in, kSyntax);
      return;
    }
    if (ch == '\n' || prev != ' ') return;  // inside "shot" or a token: checked by its first byte
    const int sect = ch == 'M' ? 0 : (ch == 'D' ? 1 : (ch == 'L' ? 2 : -1));
    if (sect < 0) {
      fault_at(a.res, i, kPrefix);
      return;
    }
    const int lo = sect == 0 ? 0 : (sect == 1 ? a.nm : a.nm + a.nd);
    const int hi = sect == 0 ? a.nm : (sect == 1 ? a.nm + a.nd : a.bits);
    if (i + 1 == a.n_in) {
      if (a.final_chunk) fault_at(a.res, a.n_in, kSyntax);
      return;
    }
    const uint8_t c1 = a.in[i + 1];
    if (c1 == ' ' || c1 == '\n') {
      fault_at(a.res, i + 1, kSyntax);  // a prefix without an index
      return;
    }
    long long v, stop;
    bool inc;
    if (!parse_index(a, i + 1, true, v, stop, inc) || inc) return;
    if (v >= (long long)(hi - lo)) {
      fault_at(a.res, i, kRange);
      return;
    }
    const int col = lo + (int)v;
    if (r < rows) set_bit(a, r, col);
  }
}

}  // namespace sdk
