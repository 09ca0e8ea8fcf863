// refuse_outputs.cpp - the host side of the column-list handles (tsim_m2d, tsim_affine, tsim_frame, tsim_faults) and of the
// union-find create calls, on a machine without a GPU: every refusal of the create and request calls, each alone, inputs wrong
// in two ways (the first refusal must stay the first), and valid descriptors that reach the window builder before the device
// is refused.  One line "name | code | text" per call; the lines of two trees' builds are compared with diff.  The window plan
// and the per-window CSR are restated here by brute force; a tree that has csrc/tsim_outputs_host.hip.h is held against them.
//
// A request call needs a handle, and no handle can be created without a device, so the program is built in parts: PART_MAIN
// (main, tsim_fail, the union-find calls, the plan and the builder) and one part per handle, which takes the handle's .hip file
// in as text and fills a handle by hand.  TREE: the repository's root (or a parent commit's checkout), out: any directory.
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//      -Xarch_host -fno-sanitize-recover=undefined -I$TREE/include -I$TREE/tsim_amd/csrc"
//   for p in MAIN M2D AFFINE FRAME FAULTS; do hipcc $F -DPART_$p -c scripts/host_checks/refuse_outputs.cpp -o out/part_$p.o; done
//   for u in uf ufw; do hipcc $F -c $TREE/tsim_amd/csrc/tsim_$u.hip -o out/tsim_$u.o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined out/part_*.o out/tsim_uf.o out/tsim_ufw.o -o out/refuse_outputs
//   out/refuse_outputs > out/lines.txt      (plain program, nothing preloaded, on the CPU)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if __has_include("tsim_outputs_host.hip.h")
#define SHARED_HOST 1
#else
#define SHARED_HOST 0
#endif

void report(const char *name, int rc);  // one line; the text of the last tsim_fail when rc < 0
void part_m2d();
void part_affine();
void part_frame();
void part_faults();

namespace {
constexpr int kNoDevice = 99;
uint8_t g_buf[64];  // a non-NULL "device" pointer: no call that gets it reaches a launch
#define CALL(name, expr) report(name, (expr))

// 70 outputs over M columns: columns on both sides of every seam of windows of 2048, the first and the last, one list empty
[[maybe_unused]] void seam_lists(int32_t M, std::vector<int32_t> *row_ptr, std::vector<int32_t> *cols, std::vector<uint8_t> *ref) {
  row_ptr->assign(1, 0);
  cols->clear();
  uint32_t x = 12345u + (uint32_t)M;
  for (int j = 0; j < 70; ++j) {
    if (j != 5 && M > 0) {
      for (int32_t s = 2048 * (1 + j % 3); s < M; s += 3 * 2048) cols->push_back(s - (j & 1));
      cols->push_back(j % 2 ? 0 : M - 1);
      for (int k = 0; k < j % 7; ++k) cols->push_back((int32_t)((x = x * 1664525u + 1013904223u) % (uint32_t)M));
      if (j == 9) cols->push_back(cols->back());  // listed twice
    }
    row_ptr->push_back((int32_t)cols->size());
  }
  ref->assign(70, 1);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef PART_M2D
#include "tsim_m2d.hip"

static void set(tsim_m2d &h, int32_t M, int32_t n_out) {
  h.device = 0;
#if SHARED_HOST
  h.o.M = M, h.o.n_out = n_out, h.o.win = 64, h.o.n_win = 1;
#else
  h.M = M, h.n_out = n_out, h.win = 64, h.n_win = 1;
#endif
}

void part_m2d() {
  tsim_m2d *out = nullptr;
  const int32_t rp[4] = {0, 1, 2, 3}, rp1[4] = {1, 1, 2, 3}, rpd[4] = {0, 2, 1, 3}, cl[3] = {0, 5, 9}, cneg[3] = {0, -1, 9}, cbig[3] = {0, 10, 9};
  const uint8_t ref[3] = {0, 1, 0};
  CALL("m2d_create out NULL", tsim_m2d_create(kNoDevice, 10, 3, rp, cl, ref, nullptr));
  CALL("m2d_create M < 0", tsim_m2d_create(kNoDevice, -1, 3, rp, cl, ref, &out));
  CALL("m2d_create n_out < 0", tsim_m2d_create(kNoDevice, 10, -1, rp, cl, ref, &out));
  CALL("m2d_create row_ptr NULL", tsim_m2d_create(kNoDevice, 10, 3, nullptr, cl, ref, &out));
  CALL("m2d_create ref NULL", tsim_m2d_create(kNoDevice, 10, 3, rp, cl, nullptr, &out));
  CALL("m2d_create row_ptr[0]", tsim_m2d_create(kNoDevice, 10, 3, rp1, cl, ref, &out));
  CALL("m2d_create row_ptr decreases", tsim_m2d_create(kNoDevice, 10, 3, rpd, cl, ref, &out));
  CALL("m2d_create cols NULL", tsim_m2d_create(kNoDevice, 10, 3, rp, nullptr, ref, &out));
  CALL("m2d_create col < 0", tsim_m2d_create(kNoDevice, 10, 3, rp, cneg, ref, &out));
  CALL("m2d_create col >= M", tsim_m2d_create(kNoDevice, 10, 3, rp, cbig, ref, &out));
  std::vector<int32_t> zero(258, 0);
  std::vector<uint8_t> ref257(257, 0);
  CALL("m2d_create too many windows", tsim_m2d_create(kNoDevice, 0x7FFFFFFF, 257, zero.data(), nullptr, ref257.data(), &out));
  CALL("m2d_create 2x: sizes, out NULL", tsim_m2d_create(kNoDevice, -1, 3, rp, cl, ref, nullptr));
  CALL("m2d_create 2x: row_ptr[0], col", tsim_m2d_create(kNoDevice, 10, 3, rp1, cbig, ref, &out));
  CALL("m2d_create 2x: col, device -1", tsim_m2d_create(-1, 10, 3, rp, cneg, ref, &out));
  CALL("m2d_create valid, device 99", tsim_m2d_create(kNoDevice, 10, 3, rp, cl, ref, &out));
  CALL("m2d_create valid, device -1", tsim_m2d_create(-1, 10, 3, rp, cl, ref, &out));
  CALL("m2d_create no output", tsim_m2d_create(kNoDevice, 10, 0, rp, nullptr, nullptr, &out));
  std::vector<int32_t> srp, sc;
  std::vector<uint8_t> sref;
  for (int32_t M : {7616, 7617}) {
    seam_lists(M, &srp, &sc, &sref);
    CALL(M == 7616 ? "m2d_create 7616 columns" : "m2d_create 7617 columns", tsim_m2d_create(kNoDevice, M, 70, srp.data(), sc.data(), sref.data(), &out));
  }
  if (out) std::abort();

  tsim_m2d h, h0;
  set(h, 100, 10);
  set(h0, 0, 10);
  uint8_t *p = g_buf;
  CALL("m2d_convert_device h NULL", tsim_m2d_convert_device(nullptr, p, 64, 13, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device B < 0", tsim_m2d_convert_device(&h, p, -1, 13, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device col0 < 0", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 2, 1, -1, 10, nullptr));
  CALL("m2d_convert_device n_cols < 0", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 2, 1, 0, -1, nullptr));
  CALL("m2d_convert_device range", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 2, 1, 3, 8, nullptr));
  CALL("m2d_convert_device in_rb packed", tsim_m2d_convert_device(&h, p, 64, 12, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device in_rb bytes", tsim_m2d_convert_device(&h, p, 64, 99, 0, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device in_rb 2^31", tsim_m2d_convert_device(&h, p, 64, 0x80000000ll, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device out_rb packed", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 1, 1, 0, 10, nullptr));
  CALL("m2d_convert_device out_rb bytes", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 9, 0, 0, 10, nullptr));
  CALL("m2d_convert_device out_rb 2^31", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 0x80000000ll, 1, 0, 10, nullptr));
  CALL("m2d_convert_device B = 0", tsim_m2d_convert_device(&h, nullptr, 0, 13, 1, nullptr, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device n_cols = 0", tsim_m2d_convert_device(&h, nullptr, 64, 13, 1, nullptr, 0, 1, 10, 0, nullptr));
  CALL("m2d_convert_device d_out NULL", tsim_m2d_convert_device(&h, p, 64, 13, 1, nullptr, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device d_meas NULL", tsim_m2d_convert_device(&h, nullptr, 64, 13, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device d_meas NULL, M = 0", tsim_m2d_convert_device(&h0, nullptr, 64, 0, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device valid", tsim_m2d_convert_device(&h, p, 64, 13, 1, p, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert_device 2x: B, range", tsim_m2d_convert_device(&h, p, -1, 13, 1, p, 2, 1, 3, 8, nullptr));
  CALL("m2d_convert_device 2x: range, in_rb", tsim_m2d_convert_device(&h, p, 64, 12, 1, p, 2, 1, 3, 8, nullptr));
  CALL("m2d_convert_device 2x: in_rb, out_rb", tsim_m2d_convert_device(&h, p, 64, 12, 1, p, 1, 1, 0, 10, nullptr));
  CALL("m2d_convert_device 2x: out_rb, NULL", tsim_m2d_convert_device(&h, p, 64, 13, 1, nullptr, 1, 1, 0, 10, nullptr));
  CALL("m2d_convert_device 2x: B = 0, out_rb", tsim_m2d_convert_device(&h, p, 0, 13, 1, p, 1, 1, 0, 10, nullptr));
  CALL("m2d_convert_device 2x: B = 0, NULL", tsim_m2d_convert_device(&h, nullptr, 0, 13, 1, nullptr, 2, 1, 0, 10, nullptr));
  CALL("m2d_convert h NULL", tsim_m2d_convert(nullptr, p, 64, 13, 1, p, 2, 1, 0, 10));
  CALL("m2d_convert range", tsim_m2d_convert(&h, p, 64, 13, 1, p, 2, 1, 3, 8));
  CALL("m2d_convert in_rb", tsim_m2d_convert(&h, p, 64, 12, 1, p, 2, 1, 0, 10));
  CALL("m2d_convert B = 0", tsim_m2d_convert(&h, nullptr, 0, 13, 1, nullptr, 2, 1, 0, 10));
  CALL("m2d_convert out NULL", tsim_m2d_convert(&h, p, 64, 13, 1, nullptr, 2, 1, 0, 10));
  CALL("m2d_convert valid", tsim_m2d_convert(&h, p, 64, 13, 1, p, 2, 1, 0, 10));
}
#endif

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef PART_AFFINE
#include "tsim_affine.hip"

static void set(tsim_affine &h, int32_t num_f, int32_t n_random, int32_t n_out) {
  h.device = 0, h.num_f = num_f, h.n_random = n_random;
#if SHARED_HOST
  h.o.M = num_f + n_random, h.o.n_out = n_out, h.o.win = 128, h.o.n_win = 1;
#else
  h.n_out = n_out, h.win = 128, h.n_win = 1;
#endif
}

void part_affine() {
  tsim_affine *out = nullptr;
  const int32_t rp[4] = {0, 1, 2, 3}, rp1[4] = {1, 1, 2, 3}, rpd[4] = {0, 2, 1, 3}, cl[3] = {0, 5, 9}, cneg[3] = {0, -1, 9}, cbig[3] = {0, 10, 9};
  const uint8_t flip[3] = {0, 1, 0};
  CALL("affine_create out NULL", tsim_affine_create(kNoDevice, 6, 4, 3, rp, cl, flip, nullptr));
  CALL("affine_create num_f < 0", tsim_affine_create(kNoDevice, -1, 4, 3, rp, cl, flip, &out));
  CALL("affine_create n_random < 0", tsim_affine_create(kNoDevice, 6, -4, 3, rp, cl, flip, &out));
  CALL("affine_create n_out < 0", tsim_affine_create(kNoDevice, 6, 4, -3, rp, cl, flip, &out));
  CALL("affine_create columns 2^31", tsim_affine_create(kNoDevice, 0x7FFFFFC0, 1, 3, rp, cl, flip, &out));
  CALL("affine_create row_ptr NULL", tsim_affine_create(kNoDevice, 6, 4, 3, nullptr, cl, flip, &out));
  CALL("affine_create flip NULL", tsim_affine_create(kNoDevice, 6, 4, 3, rp, cl, nullptr, &out));
  CALL("affine_create row_ptr[0]", tsim_affine_create(kNoDevice, 6, 4, 3, rp1, cl, flip, &out));
  CALL("affine_create row_ptr decreases", tsim_affine_create(kNoDevice, 6, 4, 3, rpd, cl, flip, &out));
  CALL("affine_create cols NULL", tsim_affine_create(kNoDevice, 6, 4, 3, rp, nullptr, flip, &out));
  CALL("affine_create col < 0", tsim_affine_create(kNoDevice, 6, 4, 3, rp, cneg, flip, &out));
  CALL("affine_create col >= M", tsim_affine_create(kNoDevice, 6, 4, 3, rp, cbig, flip, &out));
  std::vector<int32_t> zero(258, 0);
  std::vector<uint8_t> f257(257, 0);
  CALL("affine_create too many windows", tsim_affine_create(kNoDevice, 0x40000000, 0x3FFFFFC0, 257, zero.data(), nullptr, f257.data(), &out));
  CALL("affine_create 2x: sizes, out NULL", tsim_affine_create(kNoDevice, -1, 4, 3, rp, cl, flip, nullptr));
  CALL("affine_create 2x: decreases, col", tsim_affine_create(kNoDevice, 6, 4, 3, rpd, cbig, flip, &out));
  CALL("affine_create 2x: col, device -1", tsim_affine_create(-1, 6, 4, 3, rp, cbig, flip, &out));
  CALL("affine_create valid, device 99", tsim_affine_create(kNoDevice, 6, 4, 3, rp, cl, flip, &out));
  CALL("affine_create valid, device -1", tsim_affine_create(-1, 6, 4, 3, rp, cl, flip, &out));
  std::vector<int32_t> srp, sc;
  std::vector<uint8_t> sref;
  for (int32_t M : {7616, 7617}) {
    seam_lists(M, &srp, &sc, &sref);
    CALL(M == 7616 ? "affine_create 7616 columns" : "affine_create 7617 columns",
         tsim_affine_create(kNoDevice, 4000, M - 4000, 70, srp.data(), sc.data(), sref.data(), &out));
  }
  if (out) std::abort();

  tsim_affine h, h0;
  set(h, 100, 20, 10);
  set(h0, 0, 20, 10);
  uint8_t *p = g_buf;
  const uint64_t *f = reinterpret_cast<const uint64_t *>(g_buf);
  const int64_t top = 1ll << 38;
  CALL("affine_sample h NULL", tsim_affine_sample_device(nullptr, f, 16, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample B < 0", tsim_affine_sample_device(&h, f, 16, -1, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample first_shot < 0", tsim_affine_sample_device(&h, f, 16, 64, -64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample first_shot % 64", tsim_affine_sample_device(&h, f, 16, 64, 63, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample first_shot > 2^38", tsim_affine_sample_device(&h, f, 16, 0, top + 64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample first_shot + B > 2^38", tsim_affine_sample_device(&h, f, 16, 65, top - 64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample first_shot + B = 2^38", tsim_affine_sample_device(&h, f, 16, 64, top - 64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample col0 < 0", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 2, 1, -1, 10, nullptr));
  CALL("affine_sample n_cols < 0", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 2, 1, 0, -1, nullptr));
  CALL("affine_sample range", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("affine_sample f_rb", tsim_affine_sample_device(&h, f, 12, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample f_rb 2^31", tsim_affine_sample_device(&h, f, 0x80000000ll, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample out_rb packed", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 1, 1, 0, 10, nullptr));
  CALL("affine_sample out_rb bytes", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 9, 0, 0, 10, nullptr));
  CALL("affine_sample out_rb 2^31", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, p, 0x80000000ll, 1, 0, 10, nullptr));
  CALL("affine_sample B = 0", tsim_affine_sample_device(&h, nullptr, 16, 0, 0, 1, 2, nullptr, 2, 1, 0, 10, nullptr));
  CALL("affine_sample n_cols = 0", tsim_affine_sample_device(&h, nullptr, 16, 64, 0, 1, 2, nullptr, 0, 1, 10, 0, nullptr));
  CALL("affine_sample d_out NULL", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, nullptr, 2, 1, 0, 10, nullptr));
  CALL("affine_sample d_f NULL", tsim_affine_sample_device(&h, nullptr, 16, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample d_f NULL, num_f = 0", tsim_affine_sample_device(&h0, nullptr, 0, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample valid", tsim_affine_sample_device(&h, f, 16, 64, 128, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample 2x: B, first_shot", tsim_affine_sample_device(&h, f, 16, -1, 63, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("affine_sample 2x: first_shot, range", tsim_affine_sample_device(&h, f, 16, 64, 63, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("affine_sample 2x: 2^38, range", tsim_affine_sample_device(&h, f, 16, 65, top - 64, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("affine_sample 2x: range, f_rb", tsim_affine_sample_device(&h, f, 12, 64, 0, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("affine_sample 2x: f_rb, out_rb", tsim_affine_sample_device(&h, f, 12, 64, 0, 1, 2, p, 1, 1, 0, 10, nullptr));
  CALL("affine_sample 2x: out_rb, NULL", tsim_affine_sample_device(&h, f, 16, 64, 0, 1, 2, nullptr, 1, 1, 0, 10, nullptr));
  CALL("affine_sample 2x: B = 0, f_rb", tsim_affine_sample_device(&h, f, 12, 0, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
}
#endif

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef PART_FRAME
#include "tsim_frame.hip"

namespace {
// H 0 | noise site 0 (one X bit on qubit 0) | M 0 -> record 0; two records, one random symbol, two outputs
struct FrameCase {
  uint8_t op_kind[3] = {frmk::kH, frmk::kNoise, frmk::kMeasure};
  int32_t op_a[3] = {0, 0, 0}, op_b[3] = {0, 0, 0}, op_c[3] = {0, 0, 0}, batch_ptr[4] = {0, 1, 2, 3};
  int32_t site_chan[1] = {0}, site_table[1] = {0}, site_bit[2] = {0, 1}, bit_ptr[3] = {0, 1, 1}, targets[2] = {0, 0};
  int32_t table_ptr[3] = {0, 1, 1}, table_gap[2] = {0, 0};
  uint32_t out_vals[2] = {1, 1}, out_thr[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, gap_thr[64];
  uint8_t out_const[2] = {0, 1};
  int32_t out_ptr[3] = {0, 1, 2}, out_cols[2] = {0, 2};
  tsim_frame_desc d{};
  FrameCase() {
    for (int k = 0; k < 64; ++k) gap_thr[k] = 0xF0000000u - 1000u * k;
    d.n_qubits = 2, d.n_records = 2, d.n_hidden = 0, d.n_random = 1, d.n_out = 2, d.n_ops = 3, d.n_batches = 3, d.n_sites = 1;
    d.n_bits = 1, d.n_targets = 1, d.n_tables = 1, d.n_outcomes = 1, d.n_gaps = 1, d.n_cols = 2;
    d.op_kind = op_kind, d.op_a = op_a, d.op_b = op_b, d.op_c = op_c, d.batch_ptr = batch_ptr;
    d.site_chan = site_chan, d.site_table = site_table, d.site_bit = site_bit, d.bit_ptr = bit_ptr, d.targets = targets;
    d.table_ptr = table_ptr, d.table_gap = table_gap, d.out_vals = out_vals, d.out_thr = out_thr, d.gap_thr = gap_thr;
    d.out_const = out_const, d.out_ptr = out_ptr, d.out_cols = out_cols;
  }
};

template <class Change>
void frame_case(const char *name, Change change, int device = kNoDevice) {
  FrameCase c;
  tsim_frame *out = nullptr;
  change(c);
  CALL(name, tsim_frame_create(device, &c.d, &out));
  if (out) std::abort();
}
}  // namespace

static void set(tsim_frame &h, int32_t n_out) {
  h.device = 0, h.nq = 2, h.n_rec = 2, h.n_random = 1;
#if SHARED_HOST
  h.o.M = 3, h.o.n_out = n_out, h.o.win = 64, h.o.n_win = 1;
#else
  h.n_out = n_out, h.win = 64, h.n_win = 1;
#endif
}

void part_frame() {
  FrameCase base;
  tsim_frame *out = nullptr;
  CALL("frame_create out NULL", tsim_frame_create(kNoDevice, &base.d, nullptr));
  CALL("frame_create desc NULL", tsim_frame_create(kNoDevice, nullptr, &out));
  frame_case("frame_create no qubit", [](FrameCase &c) { c.d.n_qubits = 0; });
  frame_case("frame_create n_records < 0", [](FrameCase &c) { c.d.n_records = -1; });
  frame_case("frame_create n_cols < 0", [](FrameCase &c) { c.d.n_cols = -1; });
  frame_case("frame_create records + hidden", [](FrameCase &c) { c.d.n_hidden = 0x3FFFFFFF; });
  frame_case("frame_create records + random", [](FrameCase &c) { c.d.n_random = 0x7FFFFFC0; });
  frame_case("frame_create qubits beyond LDS", [](FrameCase &c) { c.d.n_qubits = 10241; });
  frame_case("frame_create op_kind NULL", [](FrameCase &c) { c.d.op_kind = nullptr; });
  frame_case("frame_create batch_ptr NULL", [](FrameCase &c) { c.d.batch_ptr = nullptr; });
  frame_case("frame_create out_ptr NULL", [](FrameCase &c) { c.d.out_ptr = nullptr; });
  frame_case("frame_create out_const NULL", [](FrameCase &c) { c.d.out_const = nullptr; });
  frame_case("frame_create out_cols NULL", [](FrameCase &c) { c.d.out_cols = nullptr; });
  frame_case("frame_create gap_thr NULL", [](FrameCase &c) { c.d.gap_thr = nullptr; });
  frame_case("frame_create targets NULL", [](FrameCase &c) { c.d.targets = nullptr; });
  frame_case("frame_create batch_ptr end", [](FrameCase &c) { c.batch_ptr[3] = 2; });
  frame_case("frame_create site_bit end", [](FrameCase &c) { c.site_bit[1] = 2; });
  frame_case("frame_create bit_ptr decreases", [](FrameCase &c) { c.d.n_bits = 2, c.site_bit[1] = 2, c.bit_ptr[1] = 2; });
  frame_case("frame_create table without outcome", [](FrameCase &c) { c.d.n_tables = 2; });
  frame_case("frame_create gap row of a table", [](FrameCase &c) { c.table_gap[0] = 1; });
  frame_case("frame_create thresholds decrease", [](FrameCase &c) { c.d.n_outcomes = 2, c.table_ptr[1] = 2, c.out_thr[0] = 5, c.out_thr[1] = 3; });
  frame_case("frame_create gap row increases", [](FrameCase &c) { c.gap_thr[40] = c.gap_thr[39] + 1; });
  frame_case("frame_create site without bit", [](FrameCase &c) { c.d.n_bits = 0, c.d.n_targets = 0, c.site_bit[1] = 0; });
  frame_case("frame_create table of a site", [](FrameCase &c) { c.site_table[0] = 1; });
  frame_case("frame_create outcome beyond bits", [](FrameCase &c) { c.out_vals[0] = 2; });
  frame_case("frame_create target kind", [](FrameCase &c) { c.targets[0] = 3; });
  frame_case("frame_create target qubit", [](FrameCase &c) { c.targets[0] = 4 * 2; });
  frame_case("frame_create target record", [](FrameCase &c) { c.targets[0] = 4 * 2 + 2; });
  frame_case("frame_create empty batch", [](FrameCase &c) { c.batch_ptr[1] = 0; });
  frame_case("frame_create operation kind", [](FrameCase &c) { c.op_kind[0] = 7; });
  frame_case("frame_create kinds of a batch", [](FrameCase &c) { c.batch_ptr[1] = 2, c.batch_ptr[2] = 2, c.d.n_batches = 2, c.batch_ptr[2] = 3; });
  frame_case("frame_create H qubit", [](FrameCase &c) { c.op_a[0] = 2; });
  frame_case("frame_create CX a = b", [](FrameCase &c) { c.op_kind[0] = frmk::kCX; });
  frame_case("frame_create measure record", [](FrameCase &c) { c.op_b[2] = 2; });
  frame_case("frame_create noise site", [](FrameCase &c) { c.op_a[1] = 1; });
  frame_case("frame_create two items, one qubit",
             [](FrameCase &c) { c.op_kind[1] = frmk::kH, c.op_kind[2] = frmk::kH, c.d.n_batches = 1, c.batch_ptr[1] = 3, c.d.n_sites = 0; });
  frame_case("frame_create out_ptr end", [](FrameCase &c) { c.out_ptr[2] = 1; });
  frame_case("frame_create out_ptr decreases", [](FrameCase &c) { c.out_ptr[1] = 3; });
  frame_case("frame_create out_col < 0", [](FrameCase &c) { c.out_cols[0] = -1; });
  frame_case("frame_create out_col >= M", [](FrameCase &c) { c.out_cols[1] = 3; });
  {
    FrameCase c;
    std::vector<int32_t> zero(258, 0);
    std::vector<uint8_t> k257(257, 0);
    c.d.n_random = 0x7FFFFF00, c.d.n_out = 257, c.d.n_cols = 0, c.d.out_ptr = zero.data(), c.d.out_const = k257.data();
    CALL("frame_create too many windows", tsim_frame_create(kNoDevice, &c.d, &out));
  }
  frame_case("frame_create 2x: sizes, qubits", [](FrameCase &c) { c.d.n_qubits = 10241, c.d.n_cols = -1; });
  frame_case("frame_create 2x: qubits, NULL", [](FrameCase &c) { c.d.n_qubits = 10241, c.d.out_ptr = nullptr; });
  frame_case("frame_create 2x: gap of table, gap row", [](FrameCase &c) { c.table_gap[0] = 1, c.gap_thr[40] = c.gap_thr[39] + 1; });
  frame_case("frame_create 2x: gap row, outcome bits", [](FrameCase &c) { c.gap_thr[40] = c.gap_thr[39] + 1, c.out_vals[0] = 2; });
  frame_case("frame_create 2x: H qubit, out_col", [](FrameCase &c) { c.op_a[0] = 2, c.out_cols[1] = 3; });
  frame_case("frame_create 2x: out_col, device -1", [](FrameCase &c) { c.out_cols[1] = 3; }, -1);
  frame_case("frame_create valid, device 99", [](FrameCase &) {});
  frame_case("frame_create valid, device -1", [](FrameCase &) {}, -1);
  frame_case("frame_create no column",
             [](FrameCase &c) { c.d.n_records = 0, c.d.n_hidden = 1, c.d.n_random = 0, c.d.n_cols = 0, c.out_ptr[1] = 0, c.out_ptr[2] = 0; });
  std::vector<int32_t> srp, sc;
  std::vector<uint8_t> sref;
  for (int32_t M : {7616, 7617, 7700}) {
    FrameCase c;
    seam_lists(M, &srp, &sc, &sref);
    c.d.n_random = M - 2, c.d.n_out = 70, c.d.n_cols = (int32_t)sc.size(), c.d.out_ptr = srp.data(), c.d.out_cols = sc.data(), c.d.out_const = sref.data();
    CALL(M == 7616 ? "frame_create 7616 columns" : M == 7617 ? "frame_create 7617 columns" : "frame_create 7700 columns",
         tsim_frame_create(kNoDevice, &c.d, &out));
  }
  if (out) std::abort();

  tsim_frame h;
  set(h, 10);
  uint8_t *p = g_buf;
  const int64_t top = 1ll << 38;
  CALL("frame_sample h NULL", tsim_frame_sample_device(nullptr, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample B < 0", tsim_frame_sample_device(&h, -1, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample first_shot < 0", tsim_frame_sample_device(&h, 64, -64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample first_shot % 64", tsim_frame_sample_device(&h, 64, 32, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample first_shot > 2^38", tsim_frame_sample_device(&h, 0, top + 64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample first_shot + B > 2^38", tsim_frame_sample_device(&h, 65, top - 64, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample col0 < 0", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 2, 1, -1, 10, nullptr));
  CALL("frame_sample n_cols < 0", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 2, 1, 0, -1, nullptr));
  CALL("frame_sample range", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("frame_sample out_rb packed", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 1, 1, 0, 10, nullptr));
  CALL("frame_sample out_rb bytes", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 9, 0, 0, 10, nullptr));
  CALL("frame_sample out_rb 2^31", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 0x80000000ll, 1, 0, 10, nullptr));
  CALL("frame_sample B = 0", tsim_frame_sample_device(&h, 0, 0, 1, 2, nullptr, 2, 1, 0, 10, nullptr));
  CALL("frame_sample n_cols = 0", tsim_frame_sample_device(&h, 64, 0, 1, 2, nullptr, 0, 1, 10, 0, nullptr));
  CALL("frame_sample d_out NULL", tsim_frame_sample_device(&h, 64, 0, 1, 2, nullptr, 2, 1, 0, 10, nullptr));
  CALL("frame_sample valid", tsim_frame_sample_device(&h, 64, 128, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample 2x: B, first_shot", tsim_frame_sample_device(&h, -1, 32, 1, 2, p, 2, 1, 0, 10, nullptr));
  CALL("frame_sample 2x: first_shot, range", tsim_frame_sample_device(&h, 64, 32, 1, 2, p, 2, 1, 3, 8, nullptr));
  CALL("frame_sample 2x: range, out_rb", tsim_frame_sample_device(&h, 64, 0, 1, 2, p, 0, 1, 3, 8, nullptr));
  CALL("frame_sample 2x: out_rb, NULL", tsim_frame_sample_device(&h, 64, 0, 1, 2, nullptr, 1, 1, 0, 10, nullptr));
  CALL("frame_sample 2x: B = 0, out_rb", tsim_frame_sample_device(&h, 0, 0, 1, 2, p, 1, 1, 0, 10, nullptr));
}
#endif

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef PART_FAULTS
#include "tsim_faults.hip"

namespace {
// two classes (2 sites of one bit, 1 site of two bits) over 4 error bits and 3 outputs
struct FaultsCase {
  int32_t class_ptr[3] = {0, 2, 3}, site_e0[3] = {0, 1, 2}, table_bits[2] = {1, 2}, table_ptr[3] = {0, 1, 3}, table_gap[2] = {0, 1};
  uint32_t out_vals[3] = {1, 1, 3}, out_thr[3] = {0xFFFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  std::vector<uint32_t> gap_thr;
  int32_t col_ptr[5] = {0, 1, 2, 3, 4}, cols[4] = {0, 1, 2, 0};
  uint8_t out_const[3] = {0, 1, 0};
  tsim_faults_desc d{};
  FaultsCase() : gap_thr(2 * fltk::kGapK) {
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < fltk::kGapK; ++k) gap_thr[(size_t)g * fltk::kGapK + k] = 0xF0000000u - 1000u * (uint32_t)k;
    d.n_out = 3, d.num_e = 4, d.n_sites = 3, d.n_classes = 2, d.n_outcomes = 3, d.n_gaps = 2, d.gap_k = fltk::kGapK, d.n_cols = 4;
    d.class_ptr = class_ptr, d.site_e0 = site_e0, d.table_bits = table_bits, d.table_ptr = table_ptr, d.table_gap = table_gap;
    d.out_vals = out_vals, d.out_thr = out_thr, d.gap_thr = gap_thr.data(), d.col_ptr = col_ptr, d.cols = cols, d.out_const = out_const;
  }
};

template <class Change>
void faults_case(const char *name, Change change, int device = kNoDevice) {
  FaultsCase c;
  tsim_faults *out = nullptr;
  change(c);
  CALL(name, tsim_faults_create(device, &c.d, &out));
  if (out) std::abort();
}
}  // namespace

void part_faults() {
  FaultsCase base;
  tsim_faults *out = nullptr;
  CALL("faults_create out NULL", tsim_faults_create(kNoDevice, &base.d, nullptr));
  CALL("faults_create desc NULL", tsim_faults_create(kNoDevice, nullptr, &out));
  faults_case("faults_create n_out < 0", [](FaultsCase &c) { c.d.n_out = -1; });
  faults_case("faults_create num_e 2^31", [](FaultsCase &c) { c.d.num_e = 0x7FFFFF01; });
  faults_case("faults_create n_gaps", [](FaultsCase &c) { c.d.n_gaps = 0x7FFFFFFF / fltk::kGapK + 1; });
  faults_case("faults_create gap_k", [](FaultsCase &c) { c.d.gap_k = 64; });
  faults_case("faults_create class_ptr NULL", [](FaultsCase &c) { c.d.class_ptr = nullptr; });
  faults_case("faults_create out_const NULL", [](FaultsCase &c) { c.d.out_const = nullptr; });
  faults_case("faults_create cols NULL", [](FaultsCase &c) { c.d.cols = nullptr; });
  faults_case("faults_create site_e0 NULL", [](FaultsCase &c) { c.d.site_e0 = nullptr; });
  faults_case("faults_create table_bits NULL", [](FaultsCase &c) { c.d.table_bits = nullptr; });
  faults_case("faults_create class_ptr end", [](FaultsCase &c) { c.class_ptr[2] = 2; });
  faults_case("faults_create col_ptr end", [](FaultsCase &c) { c.col_ptr[4] = 3; });
  faults_case("faults_create class without site", [](FaultsCase &c) { c.class_ptr[1] = 0; });
  faults_case("faults_create class beyond 2^25 sites", [](FaultsCase &c) { c.d.n_sites = (1 << 25) + 2, c.class_ptr[1] = (1 << 25) + 1, c.class_ptr[2] = (1 << 25) + 2; });
  faults_case("faults_create bits of a class", [](FaultsCase &c) { c.table_bits[0] = 33; });
  faults_case("faults_create table without outcome", [](FaultsCase &c) { c.table_ptr[1] = 0; });
  faults_case("faults_create gap row of a table", [](FaultsCase &c) { c.table_gap[1] = 2; });
  faults_case("faults_create thresholds decrease", [](FaultsCase &c) { c.out_thr[2] = 1; });
  faults_case("faults_create outcome beyond bits", [](FaultsCase &c) { c.out_vals[0] = 2; });
  faults_case("faults_create site_e0 < 0", [](FaultsCase &c) { c.site_e0[1] = -1; });
  faults_case("faults_create site_e0 end", [](FaultsCase &c) { c.site_e0[2] = 3; });
  faults_case("faults_create gap row increases", [](FaultsCase &c) { c.gap_thr[fltk::kGapK + 700] += 5000; });
  faults_case("faults_create col_ptr decreases", [](FaultsCase &c) { c.col_ptr[2] = 0; });
  faults_case("faults_create col < 0", [](FaultsCase &c) { c.cols[3] = -1; });
  faults_case("faults_create col >= n_out", [](FaultsCase &c) { c.cols[3] = 3; });
  faults_case("faults_create 2x: sizes, gap_k", [](FaultsCase &c) { c.d.n_out = -1, c.d.gap_k = 64; });
  faults_case("faults_create 2x: gap_k, NULL", [](FaultsCase &c) { c.d.gap_k = 64, c.d.cols = nullptr; });
  faults_case("faults_create 2x: thresholds, outcome of the table before", [](FaultsCase &c) { c.out_thr[2] = 1, c.out_vals[0] = 2; });
  faults_case("faults_create 2x: outcome, thresholds of one table", [](FaultsCase &c) { c.out_vals[1] = 4, c.out_thr[2] = 1; });
  faults_case("faults_create 2x: site_e0, gap row", [](FaultsCase &c) { c.site_e0[2] = 3, c.gap_thr[5] += 5000; });
  faults_case("faults_create 2x: gap row, col", [](FaultsCase &c) { c.gap_thr[5] += 5000, c.cols[3] = 3; });
  faults_case("faults_create 2x: col, device -1", [](FaultsCase &c) { c.cols[3] = 3; }, -1);
  faults_case("faults_create valid, device 99", [](FaultsCase &) {});
  faults_case("faults_create valid, device -1", [](FaultsCase &) {}, -1);
  {
    FaultsCase c;
    std::vector<uint8_t> k(21000, 1);
    c.d.n_out = 21000, c.d.out_const = k.data(), c.cols[3] = 20999;
    CALL("faults_create 21000 outputs", tsim_faults_create(kNoDevice, &c.d, &out));
  }
  if (out) std::abort();

  tsim_faults h;
  h.device = 0, h.n_out = 10, h.n_sites = 5, h.n_classes = 2;
  h.class_n = {2, 3};
  uint8_t *p = g_buf;
  const int64_t top = 1ll << 38;
  for (int weight = 0; weight < 2; ++weight) {
    auto sample = [&](const char *name, tsim_faults *hh, int64_t B, int64_t first_shot, uint8_t *d_out, int64_t rb, int32_t packed, int32_t col0, int32_t n) {
      char label[96];
      std::snprintf(label, sizeof label, "%s %s", weight ? "faults_sample_weight" : "faults_sample", name);
      CALL(label, weight ? tsim_faults_sample_weight_device(hh, 1, B, first_shot, 1, 2, d_out, rb, packed, col0, n, nullptr)
                         : tsim_faults_sample_device(hh, B, first_shot, 1, 2, d_out, rb, packed, col0, n, nullptr));
    };
    if (weight) {
      CALL("faults_sample_weight no split table", tsim_faults_sample_weight_device(&h, 1, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
      h.kmax = 3;
      CALL("faults_sample_weight k < 0", tsim_faults_sample_weight_device(&h, -1, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
      CALL("faults_sample_weight k > kmax", tsim_faults_sample_weight_device(&h, 4, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
      h.n_sites = 2;
      CALL("faults_sample_weight k > sites", tsim_faults_sample_weight_device(&h, 3, 64, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
      CALL("faults_sample_weight 2x: k, B", tsim_faults_sample_weight_device(&h, 3, -1, 0, 1, 2, p, 2, 1, 0, 10, nullptr));
      h.n_sites = 5;
    }
    sample("h NULL", nullptr, 64, 0, p, 2, 1, 0, 10);
    sample("B < 0", &h, -1, 0, p, 2, 1, 0, 10);
    sample("first_shot < 0", &h, 64, -64, p, 2, 1, 0, 10);
    sample("first_shot % 64", &h, 64, 1, p, 2, 1, 0, 10);
    sample("first_shot > 2^38", &h, 0, top + 64, p, 2, 1, 0, 10);
    sample("first_shot + B > 2^38", &h, 65, top - 64, p, 2, 1, 0, 10);
    sample("col0 < 0", &h, 64, 0, p, 2, 1, -1, 10);
    sample("n_cols < 0", &h, 64, 0, p, 2, 1, 0, -1);
    sample("range", &h, 64, 0, p, 2, 1, 3, 8);
    sample("out_rb packed", &h, 64, 0, p, 1, 1, 0, 10);
    sample("out_rb bytes", &h, 64, 0, p, 9, 0, 0, 10);
    sample("out_rb 2^31", &h, 64, 0, p, 0x80000000ll, 1, 0, 10);
    sample("B = 0", &h, 0, 0, nullptr, 2, 1, 0, 10);
    sample("n_cols = 0", &h, 64, 0, nullptr, 0, 1, 10, 0);
    sample("d_out NULL", &h, 64, 0, nullptr, 2, 1, 0, 10);
    sample("valid", &h, 64, 128, p, 2, 1, 0, 10);
    sample("2x: B, first_shot", &h, -1, 1, p, 2, 1, 0, 10);
    sample("2x: first_shot, range", &h, 64, 1, p, 2, 1, 3, 8);
    sample("2x: range, out_rb", &h, 64, 0, p, 0, 1, 3, 8);
    sample("2x: out_rb, NULL", &h, 64, 0, nullptr, 1, 1, 0, 10);
    sample("2x: B = 0, out_rb", &h, 0, 0, p, 1, 1, 0, 10);
  }
  h.kmax = -1;
  std::vector<uint32_t> split(2 * 4 * 4, 0);  // kmax = 3: rows (c, r) of 4 entries; all zero is valid
  CALL("faults_set_split h NULL", tsim_faults_set_split(nullptr, 3, split.data()));
  CALL("faults_set_split kmax < 0", tsim_faults_set_split(&h, -1, split.data()));
  CALL("faults_set_split kmax > 32", tsim_faults_set_split(&h, fltk::kMaxWeight + 1, split.data()));
  CALL("faults_set_split table NULL", tsim_faults_set_split(&h, 3, nullptr));
  h.always_class = 1;
  CALL("faults_set_split a class always fires", tsim_faults_set_split(&h, 3, split.data()));
  CALL("faults_set_split 2x: kmax, always", tsim_faults_set_split(&h, -1, split.data()));
  h.always_class = -1;
  h.n_classes = 1 << 30;
  CALL("faults_set_split too many entries", tsim_faults_set_split(&h, 1, split.data()));
  h.n_classes = 2;
  split[(1 * 4 + 2) * 4 + 1] = 7;  // row (1, 2): 0 7 0 0
  CALL("faults_set_split row decreases", tsim_faults_set_split(&h, 3, split.data()));
  split[(1 * 4 + 2) * 4 + 1] = 0, split[(1 * 4 + 2) * 4 + 2] = split[(1 * 4 + 2) * 4 + 3] = 7;  // 0 0 7 7
  CALL("faults_set_split valid rows", tsim_faults_set_split(&h, 3, split.data()));
  split[(1 * 4 + 2) * 4 + 0] = split[(1 * 4 + 2) * 4 + 1] = 7;  // 7 7 7 7: class 1 is the last, 0 sites here would leave 2 to no site
  CALL("faults_set_split leaves too many", tsim_faults_set_split(&h, 3, split.data()));
  split[(0 * 4 + 1) * 4 + 1] = 9, split[(0 * 4 + 1) * 4 + 2] = 8;
  CALL("faults_set_split 2x: leaves, decreases in class 0", tsim_faults_set_split(&h, 3, split.data()));
  if (h.kmax != -1 || h.split) std::abort();
}
#endif

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef PART_MAIN
#include "tsim_hip.h"
#if SHARED_HOST
#include "tsim_outputs_host.hip.h"
#endif

static char g_text[1024];
static int g_calls = 0;

int tsim_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_text, sizeof g_text, fmt, ap);
  va_end(ap);
  return code;
}

void report(const char *name, int rc) {
  std::printf("%s | %d | %s\n", name, rc, rc < 0 ? g_text : "");
  g_text[0] = 0;
  ++g_calls;
}

// the window plan and the per-window CSR, restated: one line each, and a tree that has the shared builder must agree
static void window_case(int32_t M, int32_t min_win) {
  const int64_t padded = ((int64_t)M + 63) / 64 * 64;
  const bool one = padded * 8 + 64 * 68 + 64 <= 64 * 1024;
  const int32_t win = one ? (int32_t)(padded > min_win ? padded : min_win) : 2048, n_win = one ? 1 : (M + 2047) / 2048;
  std::vector<int32_t> rp, cl;
  std::vector<uint8_t> ref;
  seam_lists(M, &rp, &cl, &ref);
  const int32_t n_out = 70;
  // brute force: for every window and output, the output's columns inside the window in their order, made window-local
  std::vector<int32_t> wrp, wcols;
  for (int32_t w = 0; w < n_win; ++w)
    for (int32_t j = 0; j <= n_out; ++j) {
      wrp.push_back((int32_t)wcols.size());
      if (j < n_out)
        for (int32_t k = rp[j]; k < rp[j + 1]; ++k)
          if (cl[k] / win == w) wcols.push_back(cl[k] % win);
    }
  uint64_t sum = 1469598103934665603ull;
  for (int32_t v : wrp) sum = (sum ^ (uint32_t)v) * 1099511628211ull;
  for (int32_t v : wcols) sum = (sum ^ (uint32_t)v) * 1099511628211ull;
#if SHARED_HOST
  outh::Outputs o;
  outh::Lists l;
  if (o.plan(M, n_out, min_win) != (int64_t)n_win * (n_out + 1) || o.win != win || o.n_win != n_win) std::abort();
  if (o.build(rp.data(), cl.data(), &l) != 0) std::abort();
  if (n_win == 1 ? (l.row_ptr != rp.data() || l.cols != cl.data())
                 : (l.wrp != wrp || l.wcols != wcols || l.row_ptr != l.wrp.data() || l.cols != l.wcols.data()))
    std::abort();
#endif
  char name[96];
  std::snprintf(name, sizeof name, "window plan and CSR, %d columns, at least %d: %d x %d, %zu + %zu entries, %016llx", M, min_win, n_win, win,
                wrp.size(), wcols.size(), (unsigned long long)sum);
  report(name, 0);
}

static void part_uf() {
  // a chain of 41 nodes (node 0: the boundary): edges (v, v + 1), and (0, 1)
  std::vector<int32_t> u, v;
  std::vector<uint64_t> obs;
  for (int i = 0; i < 40; ++i) u.push_back(i), v.push_back(i + 1), obs.push_back(i == 0);
  std::vector<uint8_t> cap(40, 3), cap15(40, 3);
  cap15[7] = 15;
  tsim_uf_desc d{41, 40, 44, u.data(), v.data(), obs.data()};
  tsim_uf *out = nullptr;
  tsim_ufw *wout = nullptr;
  auto with = [&](auto change) {
    tsim_uf_desc c = d;
    change(c);
    return c;
  };
  std::vector<int32_t> u2 = u, v2 = v;
  tsim_uf_desc c;
  CALL("uf_create out NULL", tsim_uf_create(kNoDevice, &d, nullptr));
  CALL("uf_create desc NULL", tsim_uf_create(kNoDevice, nullptr, &out));
  c = with([](tsim_uf_desc &x) { x.n_nodes = 1; });
  CALL("uf_create n_nodes", tsim_uf_create(kNoDevice, &c, &out));
  CALL("ufw_create n_nodes", tsim_ufw_create(kNoDevice, &c, nullptr, 4, 8, &wout));
  c = with([](tsim_uf_desc &x) { x.n_edges = -1; });
  CALL("uf_create n_edges", tsim_uf_create(kNoDevice, &c, &out));
  CALL("ufw_create n_edges", tsim_ufw_create(kNoDevice, &c, nullptr, 4, 8, &wout));
  c = with([](tsim_uf_desc &x) { x.n_nodes = 65536; });
  CALL("uf_create 65536 nodes", tsim_uf_create(kNoDevice, &c, &out));
  c = with([](tsim_uf_desc &x) { x.n_cols = 39; });
  CALL("uf_create n_cols", tsim_uf_create(kNoDevice, &c, &out));
  CALL("ufw_create n_cols", tsim_ufw_create(kNoDevice, &c, nullptr, 4, 8, &wout));
  c = with([](tsim_uf_desc &x) { x.edge_obs = nullptr; });
  CALL("uf_create edge array NULL", tsim_uf_create(kNoDevice, &c, &out));
  CALL("ufw_create edge array NULL", tsim_ufw_create(kNoDevice, &c, nullptr, 4, 8, &wout));
  v2[39] = 41;
  c = with([&](tsim_uf_desc &x) { x.edge_v = v2.data(); });
  CALL("uf_create edge leaves the nodes", tsim_uf_create(kNoDevice, &c, &out));
  CALL("ufw_create edge leaves the nodes", tsim_ufw_create(kNoDevice, &c, nullptr, 4, 8, &wout));
  v2[39] = 39;
  CALL("uf_create u >= v", tsim_uf_create(kNoDevice, &c, &out));
  v2[39] = 40, u2[20] = 18;
  c = with([&](tsim_uf_desc &x) { x.edge_u = u2.data(); });
  CALL("uf_create not ascending", tsim_uf_create(kNoDevice, &c, &out));
  CALL("uf_create cap 15", tsim_uf_create_weighted(kNoDevice, &d, cap15.data(), &out));
  CALL("ufw_create cap 15", tsim_ufw_create(kNoDevice, &d, cap15.data(), 4, 8, &wout));
  CALL("ufw_create commit 0", tsim_ufw_create(kNoDevice, &d, nullptr, 0, 8, &wout));
  CALL("ufw_create window < commit", tsim_ufw_create(kNoDevice, &d, nullptr, 8, 4, &wout));
  CALL("ufw_create 2x: window, cap", tsim_ufw_create(kNoDevice, &d, cap15.data(), 8, 4, &wout));
  // heralds: 40 of them, columns 40 .. 79 after the nodes' 0 .. 39, herald i lists edge i
  std::vector<int32_t> node_det, her_det, her_ptr(1, 0), her_edges;
  for (int i = 0; i < 40; ++i) node_det.push_back(i), her_det.push_back(40 + i), her_edges.push_back(i), her_ptr.push_back(i + 1);
  tsim_uf_heralds her{80, 40, node_det.data(), her_det.data(), her_ptr.data(), her_edges.data()};
  tsim_uf_desc dh = d;
  dh.n_cols = 84;
  tsim_uf_heralds hbad = her;
  hbad.n_det_cols = 79;
  CALL("uf_create_heralds n_det_cols", tsim_uf_create_heralds(kNoDevice, &dh, cap.data(), &hbad, &out));
  CALL("ufw_create_heralds n_det_cols", tsim_ufw_create_heralds(kNoDevice, &dh, cap.data(), 4, 8, &hbad, &wout));
  hbad = her, hbad.herald_ptr = nullptr;
  CALL("uf_create_heralds herald array NULL", tsim_uf_create_heralds(kNoDevice, &dh, cap.data(), &hbad, &out));
  CALL("ufw_create_heralds herald array NULL", tsim_ufw_create_heralds(kNoDevice, &dh, cap.data(), 4, 8, &hbad, &wout));
  std::vector<int32_t> twice = her_det;
  twice[3] = 5;
  hbad = her, hbad.herald_det = twice.data();
  CALL("uf_create_heralds column twice", tsim_uf_create_heralds(kNoDevice, &dh, cap.data(), &hbad, &out));
  CALL("ufw_create_heralds column twice", tsim_ufw_create_heralds(kNoDevice, &dh, cap.data(), 4, 8, &hbad, &wout));
  // valid: the tables, windows and herald lists are built, then the device is refused
  CALL("uf_create valid", tsim_uf_create(kNoDevice, &d, &out));
  CALL("uf_create valid, device -1", tsim_uf_create(-1, &d, &out));
  CALL("uf_create_weighted valid", tsim_uf_create_weighted(kNoDevice, &d, cap.data(), &out));
  CALL("uf_create_heralds valid", tsim_uf_create_heralds(kNoDevice, &dh, cap.data(), &her, &out));
  CALL("ufw_create valid 4 / 8", tsim_ufw_create(kNoDevice, &d, nullptr, 4, 8, &wout));
  CALL("ufw_create valid, caps, one window", tsim_ufw_create(kNoDevice, &d, cap.data(), 50, 100, &wout));
  CALL("ufw_create_heralds valid 4 / 8", tsim_ufw_create_heralds(kNoDevice, &dh, cap.data(), 4, 8, &her, &wout));
  CALL("ufw_create_heralds valid, one window", tsim_ufw_create_heralds(kNoDevice, &dh, cap.data(), 50, 100, &her, &wout));
  CALL("uf_decode h NULL", tsim_uf_decode_device(nullptr, g_buf, 64, 8, nullptr, nullptr, 40, 41, nullptr, nullptr, nullptr));
  CALL("ufw_decode h NULL", tsim_ufw_decode_device(nullptr, g_buf, 64, 8, nullptr, nullptr, 40, 41, nullptr, nullptr, nullptr));
  if (out || wout) std::abort();
}

int main() {
  part_m2d();
  part_affine();
  part_frame();
  part_faults();
  part_uf();
  for (int32_t M : {0, 1, 64, 2047, 2048, 2049, 7616, 7617, 8192, 8193}) window_case(M, 0);
  window_case(0, 64);
  window_case(7616, 64);
  window_case(7700, 64);
  std::fprintf(stderr, "%d calls\n", g_calls);
  return 0;
}
#endif
