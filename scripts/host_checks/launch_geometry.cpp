// launch_geometry.cpp - the pure rules under the one-batch launcher (the LDS of a chunk-table block and its limit,
// list_geometry, many_hard_rows, max_param_words, the chunk-count choice) on a machine without a GPU: one line per case, the
// lines of two trees' builds compared with cmp.  A tree that has the shared functions (csrc/tsim_sample_internal.hip.h) is
// called through them; for a tree from before them, the expressions of its launch_over / launch_hw / flush_batch /
// launch_sample and of tsim_program.hip's kNch loop stand below, verbatim, as the program's own statement of them.
// tsim_program is filled by hand; nothing here reaches HIP.  TREE: the repository's root or a parent commit's checkout.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=undefined -I$TREE/include -I$TREE/tsim_amd/csrc
//         -c scripts/host_checks/launch_geometry.cpp -o out/launch_geometry.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined out/launch_geometry.o -o out/launch_geometry
//   out/launch_geometry > out/lines.txt      (plain program, nothing preloaded, on the CPU)
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "tsim_sample_internal.hip.h"

static char g_text[256];
int tsim_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_text, sizeof g_text, fmt, ap);
  va_end(ap);
  return code;
}

#ifndef TSIM_NCH_LIST  // a tree from before the shared functions: its expressions, copied
static size_t v4_block_lds(const tsim_program *p, int WF, int WO, int threads) {
  const int blk = threads;
  const size_t tile_bytes = std::max((size_t)p->v4_max_nch * 16, (size_t)p->v4_max_sent) * p->v4_gt * 16;
  const size_t lds4 = (size_t)(2 * WF + 2 * WO) * blk * 4 + 2 * tile_bytes;
  return lds4;
}
static int v4_lds_check(const tsim_program *p, size_t lds4) {
  if (lds4 > (p->v4_max_nch == 32 ? 160 : 64) * 1024) return tsim_fail(TSIM_ENOTSUP, "v4 kernel needs %zu B of LDS", lds4);
  return 0;
}
static long long list_geometry(long long blocks, long long grid1, int n_lists, int blk1) {
  const long long iters = (blocks + grid1 - 1) / grid1;
  const long long list_cap = (grid1 + n_lists - 1) / n_lists * iters * blk1;
  return list_cap;
}
static bool many_hard_rows(const tsim_program *p, int n_ctx) {
  const uint32_t fb_sum = p->h_feedback ? p->h_feedback[0] : 0xFFFFFFFFu;
  const bool many = fb_sum != 0xFFFFFFFFu && (unsigned long long)fb_sum * (unsigned)n_ctx > 16384ull;
  return many;
}
static int max_param_words(const tsim_program *p) {
  int wmax = 1;
  for (int w : p->comp_w) wmax = std::max(wmax, w);
  return wmax;
}
static int tsim_choose_nch(int maxp) {
  static const int kNch[] = {2, 4, 6, 8, 10, 12, 14, 16, 20, 32};
  int v4_max_nch = 32;
  for (int v : kNch)
    if (4 * v >= maxp) { v4_max_nch = v; break; }
  return v4_max_nch;
}
#endif

int main() {
  static const int kCounts[] = {0, 2, 4, 6, 8, 10, 12, 14, 16, 20, 32};
  static const int kSent[] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1024, 2048, 4095, 4096};
  static const long long kB[] = {1, 63, 64, 1023, 1024, 1025, 2500, 1ll << 20, (1ll << 32) - 1};
  tsim_program *p = new tsim_program;
  long long lines = 0;
  // the LDS of a chunk-table block and its limit
  for (int nch : kCounts)
    for (int gt : {1, 4})
      for (int sent : kSent)
        for (int threads : {256, 512})
          for (int WF = 1; WF <= 40; ++WF)
            for (int WO = 1; WO <= 5; ++WO) {
              p->v4_max_nch = nch, p->v4_gt = gt, p->v4_max_sent = sent;
              const size_t lds = v4_block_lds(p, WF, WO, threads);
              g_text[0] = 0;
              const int rc = v4_lds_check(p, lds);
              std::printf("lds nch %d gt %d sent %d threads %d WF %d WO %d | %zu | %d | %s\n", nch, gt, sent, threads, WF, WO, lds, rc, g_text);
              ++lines;
            }
  // the first pass's lists: one block per row block, or the chip's worth of blocks striding (256 CUs, 2048 threads each)
  for (long long B : kB)
    for (int block : {256, 1024})
      for (int n_lists : {1, 2, 4, 8, 16, 32, 64}) {
        const long long blocks = (B + block - 1) / block;
        for (long long grid : {blocks, std::min(blocks, 256ll * (2048 / block)), std::min(blocks, 7ll)}) {
          std::printf("lists B %lld block %d n_lists %d grid %lld | %lld\n", B, block, n_lists, grid, list_geometry(blocks, grid, n_lists, block));
          ++lines;
        }
      }
  // many hard rows: by the last launch's count and the launches of the batch
  static uint32_t fb[8];
  for (int have = 0; have < 2; ++have)
    for (uint32_t sum : {0u, 1u, 1024u, 1025u, 2048u, 2049u, 8192u, 8193u, 16384u, 16385u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu})
      for (int n_ctx = 1; n_ctx <= 16; ++n_ctx) {
        fb[0] = sum;
        p->h_feedback = have ? fb : nullptr;
        std::printf("many feedback %d sum %u n_ctx %d | %d\n", have, sum, n_ctx, many_hard_rows(p, n_ctx) ? 1 : 0);
        ++lines;
      }
  p->h_feedback = nullptr;
  // parameter words, and the chunk count by the widest level's parameters
  for (int a = 0; a <= 9; ++a)
    for (int b = 0; b <= 9; ++b) {
      p->comp_w.clear();
      if (a) p->comp_w.push_back(a);
      if (b) p->comp_w.push_back(b);
      std::printf("words %d %d | %d\n", a, b, max_param_words(p));
      ++lines;
    }
  for (int maxp = 0; maxp <= 300; ++maxp) {
    std::printf("chunks maxp %d | %d\n", maxp, tsim_choose_nch(maxp));
    ++lines;
  }
  delete p;
  std::fprintf(stderr, "%lld lines\n", lines);
  return 0;
}
