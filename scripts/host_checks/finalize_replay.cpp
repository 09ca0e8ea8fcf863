// finalize_replay.cpp - tsim_program_finalize on a machine without a GPU, under the host sanitizers: replays the C API calls
// tsim_program_create, _add_component, _add_level, _set_mode and _finalize for the programs of a binary dump
// (scripts/host_checks/finalize_dump.py writes it; format there), every program on both formulations.  The host stages of
// finalize run before the first HIP call, so every handle ends with the device's refusal; what the run shows is that the
// stages - the deferred copies of the image writer above all, whose sources must outlive the stage that queued them - touch no
// memory they should not, and, with TSIM_AMD_DEBUG=finalize,imghash (set here unless the caller set it), the image hashes and
// plan lines on stderr: the same as tests/golden/image_hashes.json and finalize_plans.json, and the same for two trees' builds.
// TREE: the repository's root (or a parent commit's checkout), out: any directory.
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//      -Xarch_host -fno-sanitize-recover=undefined -I$TREE/include -I$TREE/tsim_amd/csrc"
//   for s in $TREE/tsim_amd/csrc/*.hip; do hipcc $F -c $s -o out/$(basename $s).o; done
//   for s in $TREE/tsim_amd/csrc/*.cpp; do hipcc $F -x c++ -msse4.1 -c $s -o out/$(basename $s).o; done
//   hipcc $F -c scripts/host_checks/finalize_replay.cpp -o out/finalize_replay.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined out/*.o -o out/finalize_replay -lrccl
//   python scripts/host_checks/finalize_dump.py out/programs.bin
//   out/finalize_replay out/programs.bin 2> out/lines.txt      (plain program, nothing preloaded, on the CPU)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tsim_hip.h"

namespace {
FILE *g_in;
void need(void *dst, size_t n) {
  if (n && fread(dst, 1, n, g_in) != n) {
    fprintf(stderr, "finalize_replay: the dump ends early\n");
    exit(2);
  }
}
int32_t i32() {
  int32_t v;
  need(&v, 4);
  return v;
}
std::vector<uint8_t> blob() {
  int64_t n;
  need(&n, 8);
  std::vector<uint8_t> b((size_t)n);
  need(b.data(), b.size());
  return b;
}
template <class T>
const T *ptr(const std::vector<uint8_t> &b) { return b.empty() ? nullptr : (const T *)b.data(); }

struct Level { int32_t head[7]; std::vector<uint8_t> arr[18]; };
struct Component { int32_t n_levels; std::vector<uint8_t> outputs, f_selection; std::vector<Level> levels; };
struct Program { std::string name; int32_t num_outputs, num_detectors; std::vector<uint8_t> direct_f, flips, order; std::vector<Component> comps; };

Program read_program() {
  Program p;
  const std::vector<uint8_t> name = blob();
  p.name.assign(name.begin(), name.end());
  p.num_outputs = i32();
  p.num_detectors = i32();
  p.direct_f = blob();
  p.flips = blob();
  p.order = blob();
  p.comps.resize((size_t)i32());
  for (Component &c : p.comps) {
    c.n_levels = i32();
    c.outputs = blob();
    c.f_selection = blob();
    c.levels.resize((size_t)c.n_levels);
    for (Level &l : c.levels) {
      need(l.head, sizeof l.head);
      for (auto &a : l.arr) a = blob();
    }
  }
  return p;
}

int fails = 0;
int check(const char *what, int rc) {
  if (rc < 0) {
    fprintf(stderr, "finalize_replay: %s: %d %s\n", what, rc, tsim_last_error());
    ++fails;
  }
  return rc;
}

// 0: the host stages ran and the device was refused (or, on a machine with a GPU, the handle was finalized)
void replay(const Program &pr, int mode) {
  fprintf(stderr, "## %s %s\n", pr.name.c_str(), mode == TSIM_MODE_FAITHFUL ? "faithful" : "auto");
  tsim_program *h = nullptr;
  if (check("create", tsim_program_create(pr.num_outputs, pr.num_detectors, (int32_t)(pr.direct_f.size() / 4), ptr<int32_t>(pr.direct_f),
                                          ptr<uint8_t>(pr.flips), ptr<int32_t>(pr.order), &h)) < 0)
    return;
  for (const Component &c : pr.comps) {
    const int ci = check("add_component", tsim_program_add_component(h, (int32_t)(c.outputs.size() / 4), ptr<int32_t>(c.outputs),
                                                                      (int32_t)(c.f_selection.size() / 4), ptr<int32_t>(c.f_selection), c.n_levels));
    for (const Level &l : c.levels) {
      tsim_level_desc d;
      memset(&d, 0, sizeof d);
      d.num_graphs = l.head[0], d.n_params = l.head[1], d.ta = l.head[2], d.tb = l.head[3], d.tc = l.head[4], d.td = l.head[5];
      d.has_approx = l.head[6];
      const std::vector<uint8_t> *a = l.arr;
      d.a_phases = ptr<uint8_t>(a[0]), d.a_params = ptr<uint8_t>(a[1]), d.a_counts = ptr<int32_t>(a[2]);
      d.b_coeffs = ptr<uint8_t>(a[3]), d.b_params = ptr<uint8_t>(a[4]);
      d.c_psi_const = ptr<uint8_t>(a[5]), d.c_psi_params = ptr<uint8_t>(a[6]), d.c_phi_const = ptr<uint8_t>(a[7]), d.c_phi_params = ptr<uint8_t>(a[8]);
      d.d_alpha = ptr<uint8_t>(a[9]), d.d_alpha_params = ptr<uint8_t>(a[10]), d.d_beta = ptr<uint8_t>(a[11]), d.d_beta_params = ptr<uint8_t>(a[12]);
      d.d_counts = ptr<int32_t>(a[13]);
      d.phase_indices = ptr<uint8_t>(a[14]), d.floatfactor = ptr<int32_t>(a[15]), d.power2 = ptr<int32_t>(a[16]), d.approx = ptr<float>(a[17]);
      check("add_level", tsim_program_add_level(h, ci, &d));
    }
  }
  check("set_mode", tsim_program_set_mode(h, mode));
  const int rc = tsim_program_finalize(h, 0);
  fprintf(stderr, "## -> finalize %d %s\n", rc, rc ? tsim_last_error() : "");
  if (rc != TSIM_OK && rc != TSIM_EHIP && rc != TSIM_EINVAL) ++fails;  // (no device: hipGetDeviceCount fails, or finds none)
  tsim_program_destroy(h);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: finalize_replay programs.bin\n");
    return 2;
  }
  setenv("TSIM_AMD_DEBUG", "finalize,imghash", 0);
  const int32_t n = i32();
  for (int32_t i = 0; i < n; ++i) {
    const Program pr = read_program();
    replay(pr, TSIM_MODE_AUTO);
    replay(pr, TSIM_MODE_FAITHFUL);
  }
  fclose(g_in);
  fprintf(stderr, "finalize_replay: %d programs x 2 modes, %d unexpected results\n", (int)n, fails);
  return fails ? 1 : 0;
}
