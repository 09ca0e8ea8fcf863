// tsim_finalize.hip - tsim_program_finalize: program description -> packed image -> upload, as a sequence of stages over one
// context.  Every offset a kernel dereferences and every routing flag the launchers read is set here.  Host code
// only: no kernels are defined here.  EMISSION ORDER IS THE LAYOUT: the stages, and the pieces inside a stage, append to the
// image in the order they stand in (tests/test_packer_image.py pins the image word for word and the plan line beside it).
#include "tsim_internal.hip.h"
#include "tsim_sample_internal.hip.h"  // slot_prepare: the lanes are created before the table-build helper takes its stream
#include "tsim_lw_fastm.hip.h"
#include "tsim_kernel4w.hip.h"  // C4_SELMASK
#include "tsim_wide.hip.h"      // WR_*: the wide record
#include "tsim_gen.hip.h"       // GR_*, GC_*: the gen record

using namespace tsimk;
using namespace tsimhost;

namespace {

// ---------------------------------------------------------------------------
// the image writer
// ---------------------------------------------------------------------------
// Appends to p->img.  The bulk of the image - graph records, rows, term tables, the block-per-row kernel's row streams, the chunk
// tables - is laid out first (space reserved, zero-filled) and copied in by the pool afterwards: one thread appending 12 MB piece
// by piece was 5 of the 12 ms of a fresh C4 handle.
// LIFETIME: whatever a deferred copy refers to (copy_later's vector, what a job given to later() captures by address) must live
// in the Finalize context or in the program until run_copy_jobs() has returned - never in a stage's frame.
struct ImageWriter {
  std::vector<uint32_t> &img;
  std::vector<std::function<void()>> jobs;
  explicit ImageWriter(std::vector<uint32_t> &v) : img(v) {}
  void align(size_t n) { img.resize((img.size() + n - 1) / n * n, 0u); }
  size_t grow(size_t n) {
    const size_t o = img.size();
    img.resize(o + n, 0u);
    return o;
  }
  template <class Range>
  size_t append(const Range &r) {  // (never a range of the image itself)
    const size_t o = img.size();
    img.insert(img.end(), std::begin(r), std::end(r));
    return o;
  }
  size_t copy_later(const std::vector<uint32_t> &v) {
    const size_t o = grow(v.size());
    if (!v.empty()) jobs.push_back([this, &v, o]() { memcpy(&img[o], v.data(), v.size() * sizeof(uint32_t)); });
    return o;
  }
  void later(std::function<void()> job) { jobs.push_back(std::move(job)); }
  void run_copy_jobs() {
    tsim_parallel_for(jobs.size(), 16, [&](size_t i) { jobs[i](); });
    jobs.clear();
  }
};

// The fast formulation's pack-time algebra of one level (pre_pack_fast)
struct PrePacked { std::vector<uint32_t> tables; bool fixed = false, ok = true; int frame = 0; };
// The chunk / column tables of one level (emit_chunk_levels)
struct Emit4 { std::vector<uint32_t> recs4, tabs4, stabs4; int nch = 1, ntiles = 0, sparse_F = -1; };

// What the stages share (the OneBatch pattern of DESIGN.md 4.3)
struct Finalize {
  tsim_program *p;
  ImageWriter w;
  std::vector<PrePacked> prepacked;          // [level of the program]: deferred copies read .tables
  std::vector<std::vector<Emit4>> emitted;   // [component][level]: deferred copies read the three vectors
  bool sum_wrap = false;  // some level's reference sum cannot be ruled out to wrap int32 (pack_level_fast)
  std::vector<std::vector<std::array<int, 3>>> lw_fsel_progs;  // per component: (f index, position in f_sel, 0)
  const bool dbg = tsim_debug("finalize");
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit Finalize(tsim_program *q) : p(q), w(q->img) {}
  void mark(const char *what) {
    if (!dbg) return;
    const auto n = std::chrono::steady_clock::now();
    unsigned long long hsh = 1469598103934665603ull;  // (FNV-1a of the image so far: a packer change that must not move a word shows here)
    if (tsim_debug("imghash"))
      for (uint32_t v : p->img) hsh = (hsh ^ v) * 1099511628211ull;
    fprintf(stderr, "[tsim] finalize: %s %.2f ms (image %zu words, hash %016llx)\n", what, std::chrono::duration<double, std::milli>(n - t0).count(),
            p->img.size(), hsh);
    t0 = std::chrono::steady_clock::now();
  }
};

// ---------------------------------------------------------------------------
// pieces that several records share
// ---------------------------------------------------------------------------
bool ascending(const std::vector<int32_t> &v) {
  for (size_t j = 1; j < v.size(); ++j)
    if (v[j] <= v[j - 1]) return false;
  return true;
}
bool sequential(const HostComponent &c) { return c.n_levels == c.n_out + 1; }
// what the wide kernels take of a component: sequential, at most 8 outputs over at most TSIMK_LWW_MAX_F ascending f indices
bool wide_component_shape(const HostComponent &c) { return sequential(c) && c.n_out <= 8 && c.F <= TSIMK_LWW_MAX_F && ascending(c.f_selection); }

// C(b, n) in U arithmetic, as one 32-bit word: a value beyond 32 bits saturates to 0xFFFFFFFF or is truncated.  (The five tables
// differ on purpose: DESIGN.md 4.4.)
template <class U>
uint32_t binom32(int b, int n, bool saturate) {
  if (b < n) return 0u;
  U c = 1;
  for (int i = 1; i <= n; ++i) c = c * (U)(b - n + i) / (U)i;
  return saturate && c > (U)0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)c;
}
// the table [k][b] = C(b, k + 1), k < nk, b < nb
template <class U>
void push_binomials(std::vector<uint32_t> &out, int nk, int nb, bool saturate) {
  for (int k = 0; k < nk; ++k)
    for (int b = 0; b < nb; ++b) out.push_back(binom32<U>(b, k + 1, saturate));
}
// RANK[ordinal][f-row bit position] = C(position inside f_sel, ordinal + 1): 8 ordinals x 128 positions (f indices below 128)
void push_rank_table(std::vector<uint32_t> &out, const std::vector<int32_t> &f_selection) {
  std::vector<int> pos_in(128, -1);
  for (size_t j = 0; j < f_selection.size(); ++j) pos_in[f_selection[j]] = (int)j;
  for (int k = 0; k < 8; ++k)
    for (int q = 0; q < 128; ++q) out.push_back(binom32<unsigned long long>(pos_in[q], k + 1, false));
}
// LUT[leaf][word] = the n_out sampled bits at their final columns (leaf = the bits in sampling order, first output most significant)
template <class T>
std::vector<uint32_t> placement_lut(const T *outputs, int n_out, int words) {
  std::vector<uint32_t> lut((size_t)words << n_out, 0u);
  for (uint32_t leaf = 0; leaf < (1u << n_out); ++leaf)
    for (int i = 0; i < n_out; ++i)
      if ((leaf >> (n_out - 1 - i)) & 1u) {
        const uint32_t dst = (uint32_t)outputs[i];
        lut[(size_t)leaf * words + (dst >> 5)] |= 1u << (dst & 31u);
      }
  return lut;
}
// The direct outputs that move from f word src_word to output word dst_word, as rotate-and-mask runs: (src bit, dst bit) pairs
// sorted, consecutive pairs merged into one field; their constant flips are ORed into `flips`.
struct Run { uint32_t rot, field; };
std::vector<Run> direct_runs(const tsim_program *p, int src_word, int dst_word, uint32_t &flips) {
  std::vector<std::array<int, 2>> m;  // (src bit, dst bit) inside the words
  for (int j = 0; j < p->n_direct; ++j) {
    const int src = p->direct_f[j], dst = p->output_order[j];
    if ((src >> 5) != src_word || (dst >> 5) != dst_word) continue;
    m.push_back({src & 31, dst & 31});
    if (p->direct_flips[j]) flips |= 1u << (dst & 31);
  }
  std::sort(m.begin(), m.end());
  std::vector<Run> runs;
  for (size_t i = 0; i < m.size();) {
    size_t j = i + 1;
    while (j < m.size() && m[j][0] == m[j - 1][0] + 1 && m[j][1] == m[j - 1][1] + 1) ++j;
    const int len = (int)(j - i);
    runs.push_back({(uint32_t)((m[i][0] - m[i][1]) & 31), (len >= 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << m[i][1]});
    i = j;
  }
  return runs;
}
// Destination-major runs over the f words [0, n_src) as (f word | rotate << 8, field) pairs with the run boundaries per
// destination word (wide and gen records)
struct RunsByDst { std::vector<uint32_t> runs, runb = std::vector<uint32_t>(1, 0u), flips; };
RunsByDst runs_by_destination(const tsim_program *p, int wo32, int n_src) {
  RunsByDst r;
  r.flips.assign((size_t)wo32, 0u);
  for (int d = 0; d < wo32; ++d) {
    for (int sw = 0; sw < n_src; ++sw)
      for (const Run &run : direct_runs(p, sw, d, r.flips[(size_t)d])) {
        r.runs.push_back((uint32_t)sw | (run.rot << 8));
        r.runs.push_back(run.field);
      }
    r.runb.push_back((uint32_t)(r.runs.size() / 2));
  }
  return r;
}
// Source-major runs over four f words and two output words as (rotate | f word << 8, field of word 0, field of word 1, 0)
// (fast and fastm records)
std::vector<uint32_t> runs_by_source(const tsim_program *p, uint32_t flip[2]) {
  std::vector<uint32_t> runs;
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 2; ++d)
      for (const Run &run : direct_runs(p, s, d, flip[d])) {
        runs.push_back(run.rot | ((uint32_t)s << 8));
        runs.push_back(d == 0 ? run.field : 0u);
        runs.push_back(d == 1 ? run.field : 0u);
        runs.push_back(0u);
      }
  return runs;
}

// ---------------------------------------------------------------------------
// stage: the switches
// ---------------------------------------------------------------------------
// Switches.  Results never depend on any of them.  Public: TSIM_AMD_ADAPTIVE, TSIM_AMD_FUSED_STEPS,
// TSIM_AMD_DEEP_TABLES (and, read where they act, TSIM_AMD_MODE / _KERNEL / _PATTERN_TABLES / _PATTERN_TABLE_MB / _DEBUG).
// Everything else the launch planner can be told - the A/B parameters tests/ and scripts/ use to run two paths against
// each other - travels in ONE variable, TSIM_AMD_TUNE="key=value,key=value".
void read_knobs(tsim_program *p) {
  auto env_int = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
  const std::string tune = getenv("TSIM_AMD_TUNE") ? std::string(",") + getenv("TSIM_AMD_TUNE") + "," : std::string();
  auto tune_ll = [&](const char *key, long long dflt) -> long long {
    const std::string k = std::string(",") + key + "=";
    const size_t at = tune.find(k);
    return at == std::string::npos ? dflt : atoll(tune.c_str() + at + k.size());
  };
  p->knobs.adaptive = env_int("TSIM_AMD_ADAPTIVE", 1) != 0;
  p->knobs.fused_steps = env_int("TSIM_AMD_FUSED_STEPS", 1) != 0;
  p->knobs.deep_tables = env_int("TSIM_AMD_DEEP_TABLES", 0);
  p->knobs.defer = tune_ll("defer_hard", 1) != 0;
  p->knobs.defer_group = (int)std::max(0ll, std::min(8ll, tune_ll("defer_group", 0)));  // 0: by table size (finish_image)
  p->knobs.lw_fast = tune_ll("lw_fast", 1) != 0;
  p->knobs.wide_fused = tune_ll("wide_fused", 1) != 0;
  p->knobs.hard_wave = tune_ll("hard_wave", 1) != 0;
  p->knobs.hard_wave_rows = (int)std::max(0ll, tune_ll("hard_wave_rows", 1024));
  p->knobs.hard_inline_rows = std::max(0ll, tune_ll("hard_inline_rows", 1ll << 40));
  p->knobs.hard_comp_par = tune_ll("hard_comp_par", 1) != 0;
  p->knobs.deep_after = (unsigned long long)std::max(0ll, tune_ll("deep_after", 0));  // 0: by the estimated build time (tsim_tables_deep_after)
  p->knobs.fused_lanes = (int)std::max(0ll, std::min(4ll, tune_ll("fused_lanes", 0)));
  p->knobs.fused_max = (int)std::max(1ll, std::min((long long)TSIMK_LWM_MAX_STEPS, tune_ll("fused_max", TSIMK_LWM_MAX_STEPS)));
  {  // "fused_max=N:S": S = the fewest shots a group of more than 8 batches may hold (tsim_steps_next_group; default 2^23)
    const size_t at = tune.find(",fused_max=");
    const size_t colon = at == std::string::npos ? at : tune.find_first_of(":,", at + 1);
    if (colon != std::string::npos && tune[colon] == ':') p->knobs.fused_long_shots = std::max(0ll, atoll(tune.c_str() + colon + 1));
  }
  p->knobs.wide_tables = tune_ll("wide_tables", 1) != 0;
  p->knobs.wide_compact = tune_ll("wide_compact", 1) != 0;
  p->knobs.x3 = tune_ll("x3", 1) != 0;
  p->knobs.x4 = (int)std::max(0ll, tune_ll("x4", 32));
  p->knobs.wide_depth = (int)std::max(0ll, std::min(4ll, tune_ll("wide_depth", 4)));
  p->knobs.wide_passes = (int)std::max(1ll, std::min(16ll, tune_ll("wide_passes", 8)));
  p->knobs.gen = (int)std::max(0ll, std::min(2ll, tune_ll("gen", 1)));
  p->knobs.trie = (int)std::max(0ll, std::min(2ll, tune_ll("trie", 1)));
  p->knobs.noise_fused = tune_ll("noise_fused", 1) != 0;
  p->knobs.shallow = tune_ll("shallow", 1) != 0;
  p->knobs.hard_overflow = tune_ll("hard_overflow", 1) != 0;
}

// ---------------------------------------------------------------------------
// stage: the evaluation formulation
// ---------------------------------------------------------------------------
void choose_formulation(tsim_program *p) {
  const char *env = getenv("TSIM_AMD_MODE");
  bool fast = (p->mode != TSIM_MODE_FAITHFUL) && !(env && strcmp(env, "faithful") == 0);
  for (auto &c : p->comps)
    for (auto &lv : c.levels) fast = fast && level_fast_eligible(lv);
  p->fast = fast;
}

// ---------------------------------------------------------------------------
// stage: pack - the component, level and graph records, the rows, the fast formulation's tables
// ---------------------------------------------------------------------------
constexpr int kAgainFaithful = 1;  // pack(): not done - p->fast is off now, run the stage again (0: done, negative: refused)

// the output bookkeeping (pipeline.py:83-102)
int check_output_order(tsim_program *p) {
  int pos = p->n_direct;
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    HostComponent &c = p->comps[ci];
    if ((int)c.levels.size() != c.n_levels)
      return tsim_fail(TSIM_EINVAL, "component %zu has %zu of %d levels", ci, c.levels.size(), c.n_levels);
    for (int j = 0; j < c.n_out; ++j) {
      if (pos >= p->num_outputs || p->output_order[pos] != c.output_indices[j])
        return tsim_fail(TSIM_EINVAL, "output_order[%d] does not match component %zu output %d", pos, ci, j);
      ++pos;
    }
  }
  if (pos != p->num_outputs)
    return tsim_fail(TSIM_EINVAL, "direct entries + component outputs cover %d of %d outputs", pos, p->num_outputs);
  return 0;
}

// parameter words of a component's rows (-1: more than TSIM_MAX_PARAMS bits)
int component_words(const HostComponent &c, int *max_params = nullptr) {
  int maxP = 1;
  for (auto &lv : c.levels) maxP = std::max(maxP, lv.P);
  if (sequential(c)) maxP = std::max(maxP, c.F + c.n_out);  // sampling appends the trial bit at position F+i (< F+n_out)
  if (max_params) *max_params = maxP;
  return round_w((maxP + 31) / 32);
}

// The fast formulation's pack-time algebra of every level, the levels side by side (C4: seven levels of 16-256 graphs, 1.1-2 ms
// each even with their graphs on eight threads - one after the other they were 12 of the 21 ms of a fresh handle)
void pre_pack_fast(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<std::pair<HostLevel *, int>> jobs;
  for (auto &c : p->comps) {
    const int W = component_words(c);
    for (auto &lv : c.levels) jobs.push_back({&lv, W});
  }
  f.prepacked.resize(jobs.size());
  // (up to 16 levels at a time on the process-wide pool, each level's graphs through the same pool: tsim_pool.cpp)
  tsim_parallel_for(jobs.size(), 16, [&](size_t i) {
    PrePacked &pp = f.prepacked[i];
    if (jobs[i].second < 0) { pp.ok = true; return; }  // (reported by lay_out_component: too many parameters)
    pp.ok = pack_level_fast(*jobs[i].first, jobs[i].second, pp.tables, pp.fixed, pp.frame);
  });
}

// (an upper bound: address space only - no reallocation while the pieces are laid out)
void reserve_image(Finalize &f) {
  tsim_program *p = f.p;
  size_t need = p->img.size() + 4096, li = 0;
  for (auto &c : p->comps) {
    need += (size_t)c.F + (size_t)c.n_out + (size_t)c.n_levels * (L_WORDS + L4_WORDS) + 256;
    for (auto &lv : c.levels) {
      need += lv.graph_rec.size() + 3 * lv.rows.size() + f.prepacked[li++].tables.size() + 256;
      need += (size_t)lv.G * G4_WORDS + (size_t)((lv.G + 3) / 4) * (32 * 16 * 4 * 4 + (size_t)std::max(TSIMK_SPARSE_ENTRIES, c.F + 33) * 16) + 64;
    }
  }
  p->img.reserve(need);
}

// rows of a fast graph record in the hard-row stream: those with a constant word in front, those without
struct HwRows { uint32_t n_meta, n_plain; };
HwRows hw_rows(const uint32_t *r) {
  return {(r[GF_N01] & 0xFFFFu) + (r[GF_N01] >> 16) + (r[GF_N3H] & 0xFFFFu),
          2u * r[GF_ND] + ((r[GF_FLAGS] & TSIMK_GFLAG_LAM) ? 1u : 0u) + ((r[GF_FLAGS] & TSIMK_GFLAG_LIN) ? 1u : 0u) + 2u * (r[GF_N3H] >> 16)};
}

// One level: graph records + rows (+ term tables and the hard-row stream of the fast formulation), its level record at lr_off
int lay_out_level(Finalize &f, HostLevel &h, int W, size_t lr_off) {
  tsim_program *p = f.p;
  ImageWriter &w = f.w;
  std::vector<uint32_t> &img = p->img;
  static const std::vector<uint32_t> no_tables;
  const std::vector<uint32_t> *tables_p = &no_tables;
  bool fixed = false;
  int frame = 0;
  if (p->fast) {
    // (packed by pre_pack_fast, all levels of the program side by side)
    PrePacked &pp = f.prepacked[(size_t)p->level_off.size()];
    if (!pp.ok) {  // a table entry exceeds int32: use the faithful layout
      p->fast = false;
      return kAgainFaithful;
    }
    tables_p = &pp.tables;
    fixed = pp.fixed;
    frame = pp.frame;
  } else {
    pack_level(h, W);
  }
  const std::vector<uint32_t> &tables = *tables_p;
  // align graph records to 16 words (one s_load_dwordx16 each)
  w.align(16);
  const uint32_t goff = (uint32_t)w.grow(h.graph_rec.size());  // (copied by the job below, which also patches the offsets in)
  const uint32_t roff = (uint32_t)w.copy_later(h.rows);
  static_assert((int)G_ROWS == (int)GF_ROWS, "row offset slot is shared by both layouts");
  uint32_t toff = 0;
  if (p->fast) {
    w.align(16);  // 64-byte aligned table entries (uint4 loads)
    toff = (uint32_t)w.copy_later(tables);
    h.tt_off = toff;
    h.tt_words = (uint32_t)tables.size();
  }
  // The same rows once more as ONE stream of uniform stride per level - [const, w_0 .. w_(W-1)] per row, graph after
  // graph in the order eval_graph_fast reads them - for the wave-per-row kernel (tsim_kernel_hw.hip.h), whose lanes
  // take one ROW each (coalesced) and whose graphs then read their parities by position.
  uint32_t hw_off = 0, hw_n = 0;
  std::vector<uint32_t> hw_start;
  if (p->fast) {
    w.align(16);
    hw_start.resize((size_t)h.G);
    for (int g = 0; g < h.G; ++g) {
      const HwRows n = hw_rows(&h.graph_rec[(size_t)g * G_WORDS]);
      hw_start[(size_t)g] = hw_n;
      hw_n += n.n_meta + n.n_plain;
    }
    hw_off = (uint32_t)w.grow((size_t)hw_n * (size_t)(1 + W));
    p->hw_max_rows = std::max(p->hw_max_rows, (long long)hw_n);
  }
  {  // (behind the copies of this level's records: the offsets of the image, the row streams)
    const HostLevel *hp = &h;
    const bool fast = p->fast;
    w.later([&img, hp, goff, roff, toff, hw_off, W, fast, hs = std::move(hw_start)]() {
      const HostLevel &h = *hp;
      if (!h.graph_rec.empty()) memcpy(&img[goff], h.graph_rec.data(), h.graph_rec.size() * sizeof(uint32_t));
      for (int g = 0; g < h.G; ++g) {
        uint32_t *gr = &img[goff + (size_t)g * G_WORDS];
        const uint32_t *r = &h.graph_rec[(size_t)g * G_WORDS];
        gr[G_ROWS] = r[G_ROWS] + roff;
        if (!fast) continue;
        gr[GF_TBL] = r[GF_TBL] + toff;
        if (r[GF_TBL2]) gr[GF_TBL2] = r[GF_TBL2] + toff;
        gr[GF_HWROW] = hs[(size_t)g];
        const HwRows n = hw_rows(r);
        if (n.n_meta + n.n_plain == 0) continue;  // (a level may have no rows at all: no &h.rows[..], no memcpy from null)
        const uint32_t *src = &h.rows[r[GF_ROWS]];
        uint32_t *dst = &img[hw_off + (size_t)hs[(size_t)g] * (size_t)(1 + W)];
        memcpy(dst, src, (size_t)n.n_meta * (size_t)(1 + W) * sizeof(uint32_t));
        src += (size_t)n.n_meta * (size_t)(1 + W);
        dst += (size_t)n.n_meta * (size_t)(1 + W);
        for (uint32_t t = 0; t < n.n_plain; ++t, src += W, dst += 1 + W) {
          dst[0] = 0u;
          memcpy(dst + 1, src, (size_t)W * sizeof(uint32_t));
        }
      }
    });
  }
  uint32_t *lr = &img[lr_off];
  lr[L_G] = (uint32_t)h.G;
  lr[L_GRAPHS] = goff;
  lr[L_HWROWS] = hw_off;
  lr[L_HWN] = hw_n;
  lr[L_FLAGS] = (h.approx ? TSIMK_LFLAG_APPROX : 0u) | (fixed ? TSIMK_LFLAG_FIXED : 0u);
  lr[L_FRAME] = (uint32_t)frame;
  p->stats[1] += 1;
  p->stats[2] += fixed ? 1 : 0;
  if (p->fast && h.sum_wrap_possible) f.sum_wrap = true;
  p->stats[5] += (long long)tables.size() * 4;  // table bytes
  if (p->fast)
    for (int g = 0; g < h.G; ++g) {
      const uint32_t *r = &h.graph_rec[(size_t)g * G_WORDS];
      p->stats[3] += r[GF_N3H] >> 16;
      p->stats[4] += (r[GF_N01] & 0xFFFF) + (r[GF_N01] >> 16) + (r[GF_N3H] & 0xFFFF);
      p->stats[6] += (r[GF_FLAGS] & TSIMK_GFLAG_D_TABLED) ? 1 : 0;
    }
  lr[L_NPARAMS] = (uint32_t)h.P;
  p->level_off.push_back((int)lr_off);
  p->total_graphs += h.G;
  p->total_rows += h.n_rows;
  return 0;
}

// One component: its record, f selection, output columns, level records, then every level
int lay_out_component(Finalize &f, size_t ci) {
  tsim_program *p = f.p;
  std::vector<uint32_t> &img = p->img;
  HostComponent &c = p->comps[ci];
  int maxP = 1;
  const int W = component_words(c, &maxP);
  if (W < 0) return tsim_fail(TSIM_ENOTSUP, "component %zu needs %d parameter bits (max %d)", ci, maxP, TSIM_MAX_PARAMS);
  p->comp_w.push_back(W);
  if (!sequential(c) && c.n_out != 1) p->sampleable = false;
  uint32_t rec[C_WORDS] = {0};
  rec[C_NOUT] = (uint32_t)c.n_out;
  rec[C_F] = (uint32_t)c.F;
  rec[C_W] = (uint32_t)W;
  rec[C_NLEVELS] = (uint32_t)c.n_levels;
  rec[C_KEYBASE] = (uint32_t)p->total_keys;
  rec[C_FSEL] = (uint32_t)f.w.append(c.f_selection);
  rec[C_OUTPOS] = (uint32_t)f.w.append(c.output_indices);
  // level records, then graph records + rows of every level
  const size_t lrec = f.w.grow((size_t)c.n_levels * L_WORDS);
  rec[C_LEVELS] = (uint32_t)lrec;
  p->level_base.push_back((int)p->level_off.size());
  for (int k = 0; k < c.n_levels; ++k)
    if (int r = lay_out_level(f, c.levels[k], W, lrec + (size_t)k * L_WORDS)) return r;
  if (sequential(c)) p->total_keys += c.n_out;
  memcpy(&img[p->comp_off + ci * C_WORDS], rec, sizeof rec);
  return 0;
}

// 0: done, kAgainFaithful: the fast formulation does not hold this program (p->fast is off, call again), negative: refused.
// Everything a second run must not inherit is reset here.
int pack(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<uint32_t> &img = p->img;
  p->hw_max_rows = 0;
  f.w.jobs.clear();
  f.prepacked.clear();
  f.sum_wrap = false;
  if (int r = check_output_order(p)) return r;
  img.clear();
  img.resize(16, 0u);  // word 0..15 reserved (keeps every offset non-zero)
  p->direct_off = (int)img.size();
  for (int j = 0; j < p->n_direct; ++j) {
    img.push_back((uint32_t)p->direct_f[j] | ((p->direct_flips[j] ? 1u : 0u) << 31));
    img.push_back((uint32_t)p->output_order[j]);
  }
  p->comp_off = (int)f.w.grow(p->comps.size() * C_WORDS);
  p->total_keys = 0;
  p->sampleable = true;
  p->total_graphs = p->total_rows = 0;
  for (auto &v : p->stats) v = 0;
  p->level_off.clear();
  p->level_base.clear();
  p->comp_w.clear();
  if (p->fast) pre_pack_fast(f);
  f.mark("  levels packed (pool)");
  if (p->fast) reserve_image(f);
  for (size_t ci = 0; ci < p->comps.size(); ++ci)
    if (int r = lay_out_component(f, ci)) return r;
  {  // TSIM_AMD_MODE=strict: the exact formulation only where NO int32 operation of the reference can wrap - products
    // (lay_out_level) and the levels' running sums (pack_level_fast: sum_wrap_possible); everything else on the faithful formulation
    const char *env = getenv("TSIM_AMD_MODE");
    if (p->fast && f.sum_wrap && env && strcmp(env, "strict") == 0) {
      p->fast = false;
      return kAgainFaithful;
    }
  }
  f.mark("  records laid out");
  f.w.run_copy_jobs();
  f.mark("rows / fast formulation packed");
  return 0;
}

// ---------------------------------------------------------------------------
// stage: the chunk / column tables (v4), when every sampled component qualifies
// ---------------------------------------------------------------------------
bool chunk_tables_eligible(const tsim_program *p) {
  bool ok = !p->comps.empty();
  for (auto &c : p->comps) {
    for (auto &lv : c.levels) ok = ok && level_v4_eligible(lv);
    // more than 64 parameters (round 5, knobs.x3): only as f_sel (<= 64 bits, words 0 and 1 of x) + outcome bits of a sequential component
    int maxp = 1;
    for (auto &lv : c.levels) maxp = std::max(maxp, lv.P);
    // (81..128, or more than 64 SELECTED bits - knobs.x4, end of round 5: four words, and the first pass must be k_sample_gen)
    // Four words only for components of MANY graphs (knobs.x4 = the least number, 32): those are what k_sample_wide cannot hold
    // (column tables beyond the LDS, a chain of graphs per dense pass); a 100-bit component of 8 graphs is better off there.
    int gtot = 0;
    for (auto &lv : c.levels) gtot += lv.G;
    if (maxp > 64) ok = ok && p->knobs.x3 && sequential(c) && ((c.F <= 64 && maxp <= 80) || (p->knobs.x4 > 0 && gtot >= p->knobs.x4 && maxp <= 128));
  }
  return ok;
}
// wide components (more than 64 parameters): column tables only, for the sparse-column kernel k_sample4w.
// Needs sequential components of at most 8 outputs over at most 256 ascending f indices below 512.
// (f indices up to 2047 since round 5: the round-2 kernels k_sample4w / k_sample_lw<true> read 16 mask words - f rows of at most
// 512 bits, p->wide_big keeps them away from wider rows - k_sample_wide reads a list of the words that hold selected bits)
bool column_tables_eligible(const tsim_program *p) {
  bool wide = !p->comps.empty() && p->max_f_index < 2048;
  for (auto &c : p->comps) {
    wide = wide && wide_component_shape(c);
    for (auto &lv : c.levels) wide = wide && level_v4_eligible(lv, true);
  }
  return wide;
}

// the chunk / column tables of every level, emitted side by side (C4: 3.5 ms one after the other).  The jobs READ the image
// (their v3 records, copied first): nothing may resize it while the pool runs.
void emit_chunk_levels(Finalize &f, bool wide) {
  tsim_program *p = f.p;
  const std::vector<uint32_t> &img = p->img;
  f.emitted.assign(p->comps.size(), {});
  std::vector<std::pair<size_t, int>> ejobs;
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    HostComponent &c = p->comps[ci];
    f.emitted[ci].resize((size_t)c.n_levels);
    for (int k = 0; k < c.n_levels; ++k) {
      f.emitted[ci][(size_t)k].sparse_F = (wide || (sequential(c) && c.n_out <= 8 && c.F + c.n_out <= 64)) ? c.F : -1;
      ejobs.push_back({ci, k});
    }
  }
  f.mark("  chunk-table setup");
  tsim_parallel_for(ejobs.size(), 16, [&](size_t j) {
    const size_t ci = ejobs[j].first;
    const int k = ejobs[j].second;
    HostLevel &h = p->comps[ci].levels[(size_t)k];
    Emit4 &e = f.emitted[ci][(size_t)k];
    const uint32_t v3recs = img[(size_t)p->level_off[p->level_base[ci] + k] + L_GRAPHS];
    std::vector<uint32_t> v3copy(img.begin() + v3recs, img.begin() + v3recs + (size_t)h.G * G_WORDS);
    emit_level4(h, p->v4_gt, p->v4_max_nch, v3copy.data(), e.recs4, e.tabs4, e.nch, e.ntiles, e.sparse_F, e.stabs4);
  });
  f.mark("  chunk tables emitted (pool)");
}

// the comp4 / L4 records over what emit_chunk_levels made, and the selection masks of wide components
void assemble_chunk_records(Finalize &f, bool wide) {
  tsim_program *p = f.p;
  ImageWriter &w = f.w;
  std::vector<uint32_t> &img = p->img;
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    HostComponent &c = p->comps[ci];
    for (int k = 0; k < 8; ++k) img[p->comp4_off + ci * C4_WORDS + k] = img[p->comp_off + ci * C_WORDS + k];
    w.align(16);
    const size_t l4 = w.grow((size_t)c.n_levels * L4_WORDS);
    img[p->comp4_off + ci * C4_WORDS + C4_LEVELS] = (uint32_t)l4;
    for (int k = 0; k < c.n_levels; ++k) {
      HostLevel &h = c.levels[k];
      Emit4 &em = f.emitted[ci][(size_t)k];
      w.align(16);
      const uint32_t roff = (uint32_t)w.copy_later(em.recs4);
      w.align(16);
      const uint32_t toff = (uint32_t)w.copy_later(em.tabs4);
      w.align(16);
      const uint32_t stoff = em.stabs4.empty() ? 0u : (uint32_t)img.size();
      w.copy_later(em.stabs4);
      p->v4_max_sent = std::max(p->v4_max_sent, em.sparse_F < 0 ? 0 : (p->v4_gt > 1 ? std::max(TSIMK_SPARSE_ENTRIES, em.sparse_F + 33) : em.sparse_F + 33));
      uint32_t *lr = &img[l4 + (size_t)k * L4_WORDS];
      lr[L4_STAB] = stoff;
      lr[L4_G] = (uint32_t)h.G;
      lr[L4_NTILES] = (uint32_t)em.ntiles;
      lr[L4_TABLES] = toff;
      lr[L4_RECS] = roff;
      lr[L4_NCH] = (uint32_t)em.nch;
      lr[L4_FLAGS] = (h.approx ? TSIMK_LFLAG_APPROX : 0u) | (h.fixed ? TSIMK_LFLAG_FIXED : 0u);
      lr[L4_FRAME] = (uint32_t)h.frame;
    }
    if (wide) {  // selection masks over f bits 0..255 and, per word, the selected bits below it
      uint32_t sel[2 * TSIMK_W_SELWORDS] = {0};
      for (int v : c.f_selection)
        if (v < 32 * TSIMK_W_SELWORDS) sel[v >> 5] |= 1u << (v & 31);
      for (int k = 1; k < TSIMK_W_SELWORDS; ++k)
        sel[TSIMK_W_SELWORDS + k] = sel[TSIMK_W_SELWORDS + k - 1] + (uint32_t)__builtin_popcount(sel[k - 1]);
      w.align(16);
      const uint32_t sel_off = (uint32_t)w.append(sel);
      img[p->comp4_off + ci * C4_WORDS + C4_SELMASK] = sel_off;
    }
  }
  w.run_copy_jobs();
}

void chunk_tables(Finalize &f) {
  tsim_program *p = f.p;
  p->v4 = false;
  p->v4w = false;
  if (p->fast && p->sampleable) {
    bool ok = chunk_tables_eligible(p);
    bool wide = !ok && column_tables_eligible(p);
    const char *kenv = getenv("TSIM_AMD_KERNEL");
    if (kenv && strcmp(kenv, "v3") == 0) ok = wide = false;
    if (p->mode == TSIM_MODE_ROW_KERNEL) ok = wide = false;
    p->v4_gt = 4;
    if (ok || wide) {
      f.w.align(16);
      p->comp4_off = (int)f.w.grow(p->comps.size() * C4_WORDS);
      p->v4_max_sent = 0;
      int maxp = 1;
      for (auto &c : p->comps)
        for (auto &lv : c.levels) maxp = std::max(maxp, lv.P);
      p->v4_max_nch = tsim_choose_nch(maxp);
      if (wide) {  // no chunk tables at all, one graph per tile (column tables only)
        p->v4_max_nch = 0;
        p->v4_gt = 1;
      }
      emit_chunk_levels(f, wide);
      assemble_chunk_records(f, wide);
      p->v4 = ok;
      p->v4w = wide;
      // f rows of more than 512 bits: k_sample_wide or the row kernel, never the round-2 kernels (16 mask words)
      p->wide_big = wide && p->max_f_index >= 32 * TSIMK_W_SELWORDS;
      for (auto &c : p->comps) p->wide_big = p->wide_big || (wide && c.F > 255);  // (positions are bytes in the round-2 kernels too)
      p->v4w_resident_bytes = 0;
      if (wide)
        for (auto &c : p->comps) {
          size_t tot = 0;
          for (auto &lv : c.levels) tot += (size_t)lv.G * (size_t)(c.F + 33) * 16;
          p->v4w_resident_bytes = std::max(p->v4w_resident_bytes, tot);
        }
    }
  }
  p->stats[7] = (p->v4 ? 1 : (p->v4w ? 2 : 0)) | (f.sum_wrap ? 64 : 0);  // (emit_wide_record ORs 32 and 16 in later)
  if (f.dbg) fprintf(stderr, "[tsim] finalize: the reference's int32 sums %s\n", f.sum_wrap ? "CAN wrap on some level (sum_wrap_possible)" : "cannot wrap");
  f.mark("chunk / column tables");
}

// ---------------------------------------------------------------------------
// stage: direct outputs as a gather program (bit-field runs), for every sampling kernel
// ---------------------------------------------------------------------------
void direct_programs(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<std::array<int, 3>> de;
  for (int j = 0; j < p->n_direct; ++j) de.push_back({p->direct_f[j], p->output_order[j], p->direct_flips[j] ? 1 : 0});
  std::vector<uint32_t> prog = emit_gather_program(de);
  f.w.align(16);
  p->lw_direct_prog = (int)f.w.append(prog);
  p->lw_direct_chunks = (int)(prog.size() / 16);
  p->lw_direct_rot = 0;
  if (p->max_f_index < 128 && p->num_outputs <= 64) p->lw_direct_rot = (int)f.w.append(emit_rotmask_program(de));
}

// ---------------------------------------------------------------------------
// stage: low-weight pattern tables: plan (records + sizes); built on the device after upload
// ---------------------------------------------------------------------------
// Which table family the program takes: narrow (sets c.trie, p->lw_trie, p->narrow_big) or wide (p->lw_wide); false: none
bool pattern_tables_eligible(tsim_program *p) {
  bool want = p->lw_request < 0 ? (p->mode == TSIM_MODE_AUTO) : (p->lw_request != 0);
  if (const char *e = getenv("TSIM_AMD_PATTERN_TABLES")) want = atoi(e) != 0;
  const bool ok = want && p->sampleable && !p->comps.empty();
  bool narrow = true;
  // (F + n_out up to 80 with F <= 64 since round 5: the chunk-table kernels hold x in three words then - p->v4 says whether they took the program)
  // Components of more than TSIMK_LW_MAX_NOUT outputs (round 6): a pattern's 2^n_out thresholds no longer fit a row - their
  // tables are pruned prefix trees in chunks of three levels (tsim_trie.hip.h), walked by k_sample_gen alone.  Without chunk
  // tables (p->v4: more than 32 counted rows in some graph, say) their hard rows are the block-per-row kernel's, whose x
  // holds up to 128 parameters (k_sample_hw<4, 0>: launch_hw)
  int cw_max = 1;
  for (int w : p->comp_w) cw_max = std::max(cw_max, w);
  const bool hw_rows_ok = p->fast && cw_max <= 4 && p->num_outputs <= 128 && p->max_f_index < 2048 && p->hw_max_rows < 60000;
  p->lw_trie = false;
  for (auto &c : p->comps) {
    c.trie = (c.n_out > TSIMK_LW_MAX_NOUT && p->knobs.trie) || (p->knobs.trie == 2 && c.n_out >= 1);  // (trie=2: every component - tests)
    narrow = narrow && sequential(c) && c.n_out <= (p->knobs.trie ? 64 : TSIMK_LW_MAX_NOUT) &&
             (c.F + c.n_out <= 64 || (p->v4 && c.F <= 64 && c.F + c.n_out <= 80) || (p->v4 && p->knobs.x4 > 0 && c.F + c.n_out <= 128) ||
              (c.trie && !p->v4 && hw_rows_ok && c.F + c.n_out <= 128));
    p->lw_trie = p->lw_trie || c.trie;
  }
  if (p->lw_trie && !p->v4 && !hw_rows_ok) narrow = false;  // (nothing to serve the hard rows of a fused group)
  if (tsim_debug("tables"))
    fprintf(stderr, "[tsim] pattern tables: narrow %d trie %d (chunk tables %d, block-per-row hard rows possible %d: fast %d, x words %d, outputs %d, f index %d, rows per level %lld)\n",
            narrow ? 1 : 0, p->lw_trie ? 1 : 0, p->v4 ? 1 : 0, hw_rows_ok ? 1 : 0, p->fast ? 1 : 0, cw_max, p->num_outputs, p->max_f_index, p->hw_max_rows);
  // more than 64 selected bits somewhere in a narrow program: every first pass but k_sample_gen holds f_sel in 64 bits, and the
  // closed-form binomials of the table builder end at b = 64 (tsim_lw.hip.h) - tables to weight 4 through the [4][256]
  // table of the wide path, gen or the full kernel (launch_sample)
  p->narrow_big = false;
  if (narrow)
    for (auto &c : p->comps) p->narrow_big = p->narrow_big || c.F > 64;
  // wide components (the sparse-column kernel's programs): tables to weight TSIMK_LWW_MAX_WEIGHT in front of it
  p->lw_wide = false;
  if (ok && !narrow && p->v4w && p->max_f_index < 2048) {
    bool wide_ok = p->knobs.wide_tables;
    for (auto &c : p->comps) wide_ok = wide_ok && wide_component_shape(c);
    p->lw_wide = wide_ok;
  }
  return ok && (narrow || p->lw_wide);
}

// the LW records (selection masks and bases inline) and the (f index, position) lists of the f_sel gather programs
void emit_lw_records(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<uint32_t> &img = p->img;
  f.w.align(32);
  p->lw_off = (int)f.w.grow(p->comps.size() * LW_WORDS);
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    const HostComponent &c = p->comps[ci];
    const uint32_t *crec = &img[p->comp_off + ci * C_WORDS];
    uint32_t *r = &img[p->lw_off + ci * LW_WORDS];
    r[LW_NOUT] = (uint32_t)c.n_out;
    r[LW_F] = (uint32_t)c.F;
    r[LW_OUTPOS] = crec[C_OUTPOS];
    r[LW_KEYBASE] = crec[C_KEYBASE];
    r[LW_BASES] = (uint32_t)(p->lw_off + ci * LW_WORDS + LW_BASES_INLINE);
    f.lw_fsel_progs.push_back({});
    for (int j = 0; j < c.F; ++j) f.lw_fsel_progs.back().push_back({c.f_selection[j], j, 0});
  }
}

// The table depths (allowed, default, built now) and the budgets.  Writes nothing to the image: the shallow-start loop plans
// on the live LW records and puts them back.
void table_depths(tsim_program *p) {
  std::vector<uint32_t> &img = p->img;
  // depth: the caller's, or 5 now and up to TSIMK_LW_MAX_WEIGHT on demand (tsim_tables.hip).  Patterns are
  // stored weight by weight, so the rows most shots read (weight 0..2) are a small cache-resident prefix
  // whatever the total; the heavier tail is read rarely.
  const bool pinned = p->lw_weight_cap >= 0;
  const int hw_cap = p->lw_wide ? TSIMK_LWW_MAX_WEIGHT : TSIMK_LW_MAX_WEIGHT;
  p->lw_cap_max = pinned ? std::min(p->lw_weight_cap, hw_cap) : hw_cap;
  // (wide components: weight 4 since round 5 - C5's 2.1 GB lift the tabulated share of its rows from 43 % to 63 %, 46 -> 41 us
  // per 10^6 shots; finalize still builds weight 3 only, the rest follows in the background like every default depth.
  // `wide_depth=3` keeps the round-4 default: the deeper table then waits for deep_after rows as before)
  p->lw_cap_default = pinned ? p->lw_cap_max : std::min(p->lw_wide ? p->knobs.wide_depth : 5, p->lw_cap_max);
  p->lw_cap_now = p->lw_cap_default;
  // per component: HBM is 288 GB, and only the prefix is hot (C3's weight-6 table is 1.8 GB; wide components: C(200, 4) patterns
  // of 8 thresholds are 2.1 GB - what lifts the tabulated share of C5's shots from 43 % to 63 %; still under 1 % of the HBM)
  p->lw_budget = 4096ll << 20;
  p->lw_trie_budget = 512ll << 20;
  if (const char *e = getenv("TSIM_AMD_PATTERN_TABLE_MB")) p->lw_budget = p->lw_trie_budget = std::max(1ll, atoll(e)) << 20;
  // Start shallow: the BASELINE jobs are 10^5-10^6 shots, and a depth-5 table (C4: 195 MB, 35 ms of
  // build) pays only from ~10^8 rows on.  Finalize builds the deepest tables that cost a millisecond or two (table
  // entries x graphs per level <= 1.2e8, ~2.4e-8 ms each: C2 depth 4 in 0.7 ms, C3 depth 3, C4 depth 3 in 2.4 ms - a third of
  // its fresh handle; at depth 2 it starts 2 ms sooner, and a job enqueued in one go, whose launch plans are all drawn before
  // any deeper table lands, pays for it: 10^8 shots in 46-75 instead of 32 ms, 4.6 % of the rows hard - also with the next
  // depth alone as a first stage of the background build, measured); the default depth follows in the background, slice by slice
  // next to the first launches (tsim_tables_extend_begin in upload_and_build, tsim_tables.hip).  A caller who named a depth gets it here.
  if (!pinned && p->knobs.shallow && p->knobs.deep_tables <= 0) {
    while (p->lw_cap_now > (p->lw_wide ? 3 : 2)) {
      TsimTablePlan t;
      std::vector<uint32_t> keep(img.begin() + p->lw_off, img.begin() + p->lw_off + (long)(p->comps.size() * LW_WORDS));
      double cost = 0;
      if (tsim_tables_plan_at(p, p->lw_cap_now, p->lw_budget, p->lw_off, t))
        for (size_t ci = 0; ci < p->comps.size(); ++ci) {
          double g = 0;
          for (auto &lv : p->comps[ci].levels) g += lv.G;
          cost += (double)(p->comps[ci].trie ? std::min(t.chunks[ci], t.npat[ci] * 64) * 8 : (t.npat[ci] << p->comps[ci].n_out)) * g / (double)p->comps[ci].levels.size();
        }
      std::copy(keep.begin(), keep.end(), img.begin() + p->lw_off);
      if (cost <= 1.2e8) break;
      --p->lw_cap_now;
    }
  }
}

// Shared column table of a wide component: when the parity words of ALL graphs of all levels fit one 16-byte entry (graph g owns
// a bit field of one 32-bit word: product rows U, V, counted rows, PhasePairs index bits, lambda, linear), a row's
// Y words for every graph are ONE walk over its set bits instead of one walk per graph.  Field layout from
// bit 0: U[h2] V[h2] O1[nc] D[2 nD] lambda lin.  Offsets 0: no shared table.
void emit_shared_columns(Finalize &f, const HostComponent &c, uint32_t &ccol_off, uint32_t &crec_off) {
  tsim_program *p = f.p;
  struct Fld { int w, off, h2, nc; };
  std::vector<Fld> fl;
  int fill[4] = {0, 0, 0, 0};
  bool okc = p->knobs.wide_compact;
  for (auto &lv : c.levels)
    for (auto &fg : lv.fg) {
      const int h2 = (int)fg.us.size(), nc = (int)(fg.c0.size() + fg.c1.size() + fg.c3.size());
      const int width = 2 * h2 + nc + 2 * fg.nD + 2;
      int w = -1;
      for (int k = 0; k < 4 && w < 0 && width <= 32; ++k)
        if (fill[k] + width <= 32) w = k;
      if (w < 0) { okc = false; break; }
      fl.push_back({w, fill[w], h2, nc});
      fill[w] += width;
    }
  if (tsim_debug("pack")) {
    size_t gi = 0;
    for (size_t k = 0; k < c.levels.size(); ++k)
      for (size_t g = 0; g < c.levels[k].fg.size(); ++g, ++gi) {
        const FastGraph &fg = c.levels[k].fg[g];
        fprintf(stderr, "[tsim] wide level %zu graph %zu: product pairs %zu, counted rows %zu + %zu + %zu, PhasePairs terms %d (tabled %d), term table %u words", k, g,
                fg.us.size(), fg.c0.size(), fg.c1.size(), fg.c3.size(), fg.nD, fg.d_tabled ? 1 : 0, c.levels[k].tt_words);
        if (okc) fprintf(stderr, ", shared entry word %d bit %d", fl[gi].w, fl[gi].off);
        fprintf(stderr, "\n");
      }
  }
  if (!okc) return;
  const int F = c.F;
  std::vector<std::array<uint32_t, 4>> cc((size_t)F + 33, std::array<uint32_t, 4>{0u, 0u, 0u, 0u});
  size_t gi = 0;
  for (auto &lv : c.levels)
    for (auto &fg : lv.fg) {
      const Fld fd = fl[gi++];
      const int P = lv.P;
      auto place = [&](const std::vector<uint64_t> &m, int bit, bool cst) {
        const uint32_t b = 1u << (fd.off + bit);
        for (int i = 0; i < F && i < P; ++i)
          if ((m[(size_t)i >> 6] >> (i & 63)) & 1) cc[(size_t)i][(size_t)fd.w] ^= b;
        for (int ch = 0; ch < 2; ++ch)
          for (int v = 0; v < 16; ++v) {
            bool par = ch == 0 && cst;  // row constants ride on the first chunk's entries
            for (int bb = 0; bb < 4; ++bb) {
              const int i = F + 4 * ch + bb;
              if (((v >> bb) & 1) && i < P && ((m[(size_t)i >> 6] >> (i & 63)) & 1)) par = !par;
            }
            if (par) cc[(size_t)(F + 1 + 16 * ch + v)][(size_t)fd.w] ^= b;
          }
      };
      int bit = 0;
      for (int s = 0; s < fd.h2; ++s) place(fg.us[(size_t)s], bit++, false);
      for (int s = 0; s < fd.h2; ++s) place(fg.vs[(size_t)s], bit++, false);
      for (size_t t = 0; t < fg.c0.size(); ++t) place(fg.c0[t], bit++, fg.c0c[t] != 0);
      for (size_t t = 0; t < fg.c1.size(); ++t) place(fg.c1[t], bit++, fg.c1c[t] != 0);
      for (size_t t = 0; t < fg.c3.size(); ++t) place(fg.c3[t], bit++, fg.c3c[t] != 0);
      for (int t = 0; t < fg.nD; ++t) {  // index bits: term 0 holds the most significant pair (as emit_level4)
        place(fg.dal[(size_t)t], bit + 2 * (fg.nD - 1 - t), false);
        place(fg.dbe[(size_t)t], bit + 2 * (fg.nD - 1 - t) + 1, false);
      }
      bit += 2 * fg.nD;
      place(fg.lam, bit++, false);
      place(fg.lin, bit++, false);
    }
  f.w.align(4);
  ccol_off = (uint32_t)p->img.size();
  for (auto &e : cc) f.w.append(e);
  crec_off = (uint32_t)p->img.size();
  for (auto &fd : fl) p->img.push_back((uint32_t)fd.w | ((uint32_t)fd.off << 8) | ((uint32_t)fd.h2 << 16) | ((uint32_t)fd.nc << 24));
}

// The wide record (k_sample_wide, tsim_wide.hip.h): ONE component.  Direct outputs as rotate-and-mask runs sorted by
// destination word, constant flips per word, the placement table LUT[leaf][word] of the sampled bits (leaf = the bits
// in sampling order, first output most significant) and the mask of the words that hold component outputs.
// Several components (round 5): one record per component, one k_sample_wide pass each, in stream order.  The first
// pass writes whole rows (direct outputs + its component); the records of the later ones carry no runs and no flips
// and WR_MERGE: their passes OR the component's bits into the rows in place (words are private to a row).
// false: no further record (too many runs: nothing emitted; too many selection words: this record emitted, all dropped)
bool emit_wide_record(Finalize &f, size_t wci, int wo32) {
  tsim_program *p = f.p;
  ImageWriter &w = f.w;
  std::vector<uint32_t> &img = p->img;
  const HostComponent &c = p->comps[wci];
  const bool merge = wci > 0;
  const RunsByDst rb = runs_by_destination(p, wo32, merge ? 0 : std::min(p->max_f_index / 32 + 1, 256));
  const std::vector<uint32_t> &runs = rb.runs, &runb = rb.runb;
  if (runs.size() / 2 > TSIMK_WIDE_MAX_RUNS) return false;
  bool more = true;
  w.align(16);
  const int wr_this = (int)w.grow(WR_WORDS);
  p->wr_offs.push_back(wr_this);
  img[(size_t)wr_this + WR_MERGE] = merge ? 1u : 0u;
  img[(size_t)wr_this + WR_KEYSUB] = p->total_keys > TSIMK_LWM_KEYS ? img[p->comp_off + wci * C_WORDS + C_KEYBASE] : 0u;
  img[(size_t)wr_this + WR_BSTRIDE] = (uint32_t)p->lw_binom_stride;
  {  // the f words that hold selected bits: masks, then (selected bits in the lower words | word index << 16)
    std::vector<uint32_t> words, masks;
    for (int v : c.f_selection) {
      if (words.empty() || words.back() != (uint32_t)(v >> 5)) { words.push_back((uint32_t)(v >> 5)); masks.push_back(0u); }
      masks.back() |= 1u << (v & 31);
    }
    if (words.empty()) { words.push_back(0u); masks.push_back(0u); }
    if (words.size() > TSIMK_WIDE_SELMAX) more = false;
    const uint32_t sel_off = (uint32_t)w.append(masks);
    uint32_t below = 0;
    for (size_t k = 0; k < words.size(); ++k) {
      img.push_back(below | (words[k] << 16));
      below += (uint32_t)__builtin_popcount(masks[k]);
    }
    img[(size_t)wr_this + WR_SELN] = (uint32_t)words.size();
    img[(size_t)wr_this + WR_SELREC] = sel_off;
  }
  const uint32_t runs_off = (uint32_t)w.append(runs);
  const uint32_t runb_off = (uint32_t)w.append(runb);
  const uint32_t flips_off = (uint32_t)w.append(rb.flips);
  const uint32_t lut_off = (uint32_t)w.append(placement_lut(c.output_indices.data(), c.n_out, wo32));
  uint32_t lutmask = 0u;
  for (int dst : c.output_indices) lutmask |= 1u << (dst >> 5);
  size_t colbytes = 0;
  for (auto &lv : c.levels) colbytes += (size_t)lv.G * (size_t)(c.F + 33) * 16;
  uint32_t ccol_off = 0, crec_off = 0;
  emit_shared_columns(f, c, ccol_off, crec_off);
  uint32_t *h = &img[(size_t)wr_this];
  h[WR_NRUNS] = (uint32_t)(runs.size() / 2);
  h[WR_RUNS] = runs_off;
  h[WR_RUNB] = runb_off;
  h[WR_FLIPS] = flips_off;
  h[WR_LUT] = lut_off;
  h[WR_LUTMASK] = lutmask;
  h[WR_WO32] = (uint32_t)wo32;
  h[WR_COLBYTES] = (uint32_t)colbytes;
  h[WR_CCOL] = ccol_off;
  h[WR_CREC] = crec_off;
  p->stats[7] |= 32 | (ccol_off ? 16 : 0);  // (after chunk_tables set the word)
  {  // the term tables of every level, for a copy in LDS: (image offset, words) per level
    const uint32_t tt_rec = (uint32_t)img.size();
    uint32_t tt_total = 0;
    for (auto &lv : c.levels) {
      img.push_back(lv.tt_off);
      img.push_back((lv.tt_words + 3u) & ~3u);
      tt_total += (lv.tt_words + 3u) & ~3u;
    }
    uint32_t gtot = 0;
    for (auto &lv : c.levels) gtot += (uint32_t)lv.G;
    img[(size_t)wr_this + WR_GTOT] = gtot;
    img[(size_t)wr_this + WR_TT] = tt_rec;
    img[(size_t)wr_this + WR_TTBYTES] = tt_total * 4u;
  }
  bool one = true;
  for (int d = 0; d < wo32; ++d) one = one && runb[(size_t)d + 1] - runb[(size_t)d] <= 1u;
  if (one) {
    const uint32_t r1_off = (uint32_t)img.size();
    for (int d = 0; d < wo32; ++d) {
      const bool has = runb[(size_t)d + 1] > runb[(size_t)d];
      img.push_back(has ? runs[2 * (size_t)runb[(size_t)d]] : 0u);
      img.push_back(has ? runs[2 * (size_t)runb[(size_t)d] + 1] : 0u);
    }
    img[(size_t)wr_this + WR_RUN1] = r1_off;
  }
  return more;
}

// wide programs: the LW records' selection masks, the binomials C(b, k + 1), k < 4, b < 256 (512), one wide record per component
void emit_wide_records(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<uint32_t> &img = p->img;
  p->lw = true;
  p->lw_reg = false;
  // selection masks: the comp4 record's (16 mask words + 16 prefix counts)
  for (size_t ci = 0; ci < p->comps.size(); ++ci)
    img[p->lw_off + ci * LW_WORDS + LW_SELMASK] = img[p->comp4_off + ci * C4_WORDS + C4_SELMASK];
  f.w.align(16);
  p->lw_binom_off = (int)img.size();
  p->lw_binom_stride = 256;
  for (auto &c : p->comps)
    if (c.F > 255) p->lw_binom_stride = 512;
  push_binomials<unsigned long long>(img, 4, p->lw_binom_stride, false);
  p->wr_off = 0;
  p->wr_offs.clear();
  const int wo32 = 2 * ((p->num_outputs + 63) / 64);
  bool wide_rec_ok = !p->comps.empty() && p->comps.size() <= (size_t)p->knobs.wide_passes && wo32 >= 2 && wo32 <= 8;
  for (auto &c : p->comps) wide_rec_ok = wide_rec_ok && c.n_out >= 1 && c.n_out <= 8;
  for (size_t wci = 0; wide_rec_ok && wci < p->comps.size(); ++wci) wide_rec_ok = emit_wide_record(f, wci, wo32);
  if (!wide_rec_ok) p->wr_offs.clear();
  p->wr_off = p->wr_offs.empty() ? 0 : p->wr_offs[0];
}

// gather programs of every component's f_sel (the LDS-staged first pass)
void emit_fsel_programs(Finalize &f) {
  tsim_program *p = f.p;
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    const std::vector<uint32_t> prog = emit_gather_program(f.lw_fsel_progs[ci]);
    const uint32_t prog_off = (uint32_t)f.w.append(prog);
    p->img[p->lw_off + ci * LW_WORDS + LW_FSELP] = prog_off;
    p->img[p->lw_off + ci * LW_WORDS + LW_FSELN] = (uint32_t)(prog.size() / 16);
  }
}

// register form of the first pass (k_sample_lw_reg): selection masks over the f row and, per word, the
// number of selected bits in the lower words.  Needs ascending f_selection (then the position of an f bit
// inside f_sel is a popcount), f indices below 128 and at most 64 outputs.  And the binomial tables of the rank computation.
void emit_reg_tables(Finalize &f) {
  tsim_program *p = f.p;
  std::vector<uint32_t> &img = p->img;
  p->lw_reg = p->max_f_index < 128 && p->num_outputs <= 64 && !p->narrow_big && !p->lw_trie;
  for (auto &c : p->comps) p->lw_reg = p->lw_reg && ascending(c.f_selection);
  if (p->narrow_big) {  // the table builder's binomials C(b, k + 1), k < 8, b < 256 (the wide path's [k][256] layout, saturated:
    // a value beyond 32 bits belongs to no tabulated pattern - the plan keeps a component's patterns below 2^32 - and must
    // only compare greater than every rank)
    f.w.align(16);
    p->lw_binom_off = (int)img.size();
    push_binomials<unsigned __int128>(img, 8, 256, true);
  }
  if (!p->lw_reg) return;
  f.w.align(16);  // binomial table of the rank computation: C(b, k + 1), k < 8, b < 64
  p->lw_binom_off = (int)img.size();
  push_binomials<unsigned long long>(img, 8, 64, false);
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    uint32_t sel[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int v : p->comps[ci].f_selection) sel[v >> 5] |= 1u << (v & 31);
    for (int k = 1; k < 4; ++k) sel[4 + k] = sel[4 + k - 1] + (uint32_t)__builtin_popcount(sel[k - 1]);
    uint32_t *r = &img[p->lw_off + ci * LW_WORDS];
    r[LW_SELMASK] = (uint32_t)(p->lw_off + ci * LW_WORDS + LW_SEL_INLINE);
    memcpy(r + LW_SEL_INLINE, sel, sizeof sel);
  }
}

// the rank table and the placement table of component ci, as the fast and fastm records hold them (the output columns are
// read back from the image: the LW record's)
void emit_rank_and_lut(Finalize &f, size_t ci, uint32_t &rank_off, uint32_t &lut_off) {
  tsim_program *p = f.p;
  const HostComponent &c = p->comps[ci];
  f.w.align(16);
  rank_off = (uint32_t)p->img.size();
  push_rank_table(p->img, c.f_selection);
  const uint32_t outpos_off = p->img[p->lw_off + ci * LW_WORDS + LW_OUTPOS];
  lut_off = (uint32_t)f.w.append(placement_lut(&p->img[outpos_off], c.n_out, 2));
}

// The fast record (k_sample_lw_fast, tsim_lw_fast.hip.h): ONE component of at most 8 outputs.  Direct outputs
// as a flat list of runs (rotate right, destination masks), the rank table and the placement table.
void emit_fast_record(Finalize &f) {
  tsim_program *p = f.p;
  p->lwf_off = 0;
  if (!(p->lw_reg && p->comps.size() == 1 && p->comps[0].n_out >= 1 && p->comps[0].n_out <= TSIMK_LWF_MAX_NOUT)) return;
  uint32_t flip[2] = {0u, 0u};
  const std::vector<uint32_t> runs = runs_by_source(p, flip);
  if (runs.size() / 4 > TSIMK_LWF_MAX_RUNS) return;
  f.w.align(16);
  p->lwf_off = (int)f.w.grow(LWF_WORDS);
  const uint32_t runs_off = (uint32_t)f.w.append(runs);
  uint32_t rank_off = 0, lut_off = 0;
  emit_rank_and_lut(f, 0, rank_off, lut_off);
  uint32_t *h = &p->img[p->lwf_off];
  h[LWF_NRUNS] = (uint32_t)(runs.size() / 4);
  h[LWF_FLIP0] = flip[0];
  h[LWF_FLIP1] = flip[1];
  h[LWF_RUNS] = runs_off;
  h[LWF_RANK] = rank_off;
  h[LWF_LUT] = lut_off;
  h[LWF_NOUT] = (uint32_t)p->comps[0].n_out;
}

// The same for programs of 2..4 components of at most 8 outputs each (k_sample_lw_fastm): one rank table, base
// table and placement table per component, their LDS offsets fixed here.  Header (16 words): n_runs, flip0,
// flip1, runs offset, n_comp, LDS words; then 8 words per component: rank table, LUT (image offsets), n_out,
// (their LDS offsets are a running sum the kernel and the launcher both form).
void emit_fastm_record(Finalize &f) {
  tsim_program *p = f.p;
  p->lwfm_off = 0;
  if (!(p->lw_reg && p->comps.size() >= 2 && p->comps.size() <= TSIMK_LWFM_MAX_COMP)) return;
  for (auto &c : p->comps)
    if (!(c.n_out >= 1 && c.n_out <= TSIMK_LWF_MAX_NOUT)) return;
  uint32_t flip[2] = {0u, 0u};
  const std::vector<uint32_t> runs = runs_by_source(p, flip);
  if (runs.size() / 4 > TSIMK_LWF_MAX_RUNS) return;
  f.w.align(16);
  p->lwfm_off = (int)f.w.grow(16 + 8 * TSIMK_LWFM_MAX_COMP);
  const uint32_t runs_off = (uint32_t)f.w.append(runs);
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    uint32_t rank_off = 0, lut_off = 0;
    emit_rank_and_lut(f, ci, rank_off, lut_off);
    uint32_t *hc = &p->img[p->lwfm_off + 16 + 8 * ci];
    hc[0] = rank_off;
    hc[1] = lut_off;
    hc[2] = (uint32_t)p->comps[ci].n_out;
  }
  uint32_t *h = &p->img[p->lwfm_off];
  h[0] = (uint32_t)(runs.size() / 4);
  h[1] = flip[0];
  h[2] = flip[1];
  h[3] = runs_off;
  h[4] = (uint32_t)p->comps.size();
}

// The gen record (k_sample_gen, tsim_gen.hip.h): ANY narrow program - f rows of up to 2048 bits, up to 512 outputs,
// up to TSIMK_GEN_MAX_COMP components, up to TSIMK_GEN_KEYS compiled outputs.  Direct-output runs sorted by destination
// word in groups of four (one scalar load each), the constant flips, a record per component, per component the
// (f word, selection mask, selected bits below) records of the words that hold selected bits and the output columns;
// RANK[ordinal][position inside f_sel] of every component as one block the kernel copies to LDS.
void emit_gen_record(Finalize &f) {
  tsim_program *p = f.p;
  ImageWriter &w = f.w;
  std::vector<uint32_t> &img = p->img;
  p->gr_off = 0;
  const int wo32 = 2 * ((p->num_outputs + 63) / 64);
  const int wf32 = (p->max_f_index >> 5) + 1;
  bool okg = p->num_outputs >= 1 && wo32 <= 16 && p->max_f_index < 2048 && (int)p->comps.size() <= TSIMK_GEN_MAX_COMP &&
             p->total_keys >= 1 && p->total_keys <= TSIMK_GEN_KEYS;
  for (auto &c : p->comps) okg = okg && ascending(c.f_selection);
  if (!okg) return;
  const RunsByDst rb = runs_by_destination(p, wo32, wf32);
  const std::vector<uint32_t> &runs = rb.runs, &runb = rb.runb;
  if (runs.size() / 2 > TSIMK_GEN_MAX_RUNS) return;
  // LDS block: the rank tables of the components, one after the other (C(b, k + 1) truncated to 32 bits: DESIGN.md 4.4)
  std::vector<uint32_t> blk;
  std::vector<uint32_t> l_rank;
  for (auto &c : p->comps) {
    while (blk.size() % 4) blk.push_back(0u);
    l_rank.push_back((uint32_t)blk.size());
    push_binomials<unsigned long long>(blk, TSIMK_LW_MAX_WEIGHT, c.F, false);
  }
  while (blk.size() % 4) blk.push_back(0u);
  if (blk.size() * 4 > 40 * 1024) return;  // (the launcher adds the pattern bases and the waves' row buffers)
  w.align(16);
  p->gr_off = (int)w.grow(GR_WORDS);
  const uint32_t lds_src = (uint32_t)w.append(blk);
  w.align(16);
  // run groups: two runs per 32-byte group (one scalar load), every destination word's runs padded with mask 0
  const uint32_t dst_off = (uint32_t)w.grow(4 * (size_t)wo32);
  w.align(16);
  const uint32_t groups_off = (uint32_t)img.size();
  uint32_t ngroups = 0;
  for (int d = 0; d < wo32; ++d) {
    const uint32_t r0 = runb[(size_t)d], r1 = runb[(size_t)d + 1];
    const uint32_t ng = (r1 - r0 + 1u) / 2u;
    img[dst_off + 4 * (size_t)d] = ngroups;
    img[dst_off + 4 * (size_t)d + 1] = ng;
    img[dst_off + 4 * (size_t)d + 2] = rb.flips[(size_t)d];
    for (uint32_t r = r0; r < r0 + 2u * ng; ++r) {
      img.push_back(r < r1 ? (runs[2 * (size_t)r] & 255u) : 0u);
      img.push_back(r < r1 ? (runs[2 * (size_t)r] >> 8) : 0u);
      img.push_back(r < r1 ? runs[2 * (size_t)r + 1] : 0u);
      img.push_back(0u);
    }
    ngroups += ng;
  }
  w.align(16);
  const uint32_t comp_off = (uint32_t)w.grow(p->comps.size() * GC_WORDS);
  for (size_t ci = 0; ci < p->comps.size(); ++ci) {
    const HostComponent &c = p->comps[ci];
    std::vector<uint32_t> sel((size_t)wf32, 0u);
    for (int v : c.f_selection) sel[(size_t)(v >> 5)] |= 1u << (v & 31);
    w.align(16);
    const uint32_t words_off = (uint32_t)img.size();
    uint32_t below = 0, nwords = 0;
    for (int k = 0; k < wf32; ++k)
      if (sel[(size_t)k]) {
        img.push_back((uint32_t)k);
        img.push_back(sel[(size_t)k]);
        img.push_back(below);
        img.push_back(0u);
        below += (uint32_t)__builtin_popcount(sel[(size_t)k]);
        ++nwords;
      }
    w.align(16);
    const uint32_t outpos_new = (uint32_t)img.size();
    const uint32_t outpos_off = img[p->lw_off + ci * LW_WORDS + LW_OUTPOS];
    for (int i = 0; i < c.n_out; ++i) img.push_back(img[outpos_off + (uint32_t)i]);
    uint32_t *cr = &img[comp_off + ci * GC_WORDS];
    cr[GC_NOUT] = (uint32_t)c.n_out;
    cr[GC_F] = (uint32_t)c.F;
    cr[GC_KEYBASE] = img[p->lw_off + ci * LW_WORDS + LW_KEYBASE];
    cr[GC_NWORDS] = nwords;
    cr[GC_WORDREC] = words_off;
    cr[GC_L_RANK] = l_rank[ci];
    cr[GC_OUTPOS] = outpos_new;
    bool affine = c.n_out > 0;
    for (int i = 1; i < c.n_out; ++i) affine = affine && img[outpos_off + (uint32_t)i] == img[outpos_off] + (uint32_t)i;
    cr[GC_OUTBASE] = affine ? img[outpos_off] : 0xFFFFFFFFu;
  }
  uint32_t *h = &img[p->gr_off];
  h[GR_NCOMP] = (uint32_t)p->comps.size();
  h[GR_WO32] = (uint32_t)wo32;
  h[GR_LDS_WORDS] = (uint32_t)blk.size();
  h[GR_LDS_SRC] = lds_src;
  h[GR_DST] = dst_off;
  h[GR_GROUPS] = groups_off;
  h[GR_COMP] = comp_off;
  h[GR_WF32_MIN] = (uint32_t)wf32;
}

void pattern_table_plan(Finalize &f) {
  tsim_program *p = f.p;
  p->lw = false;
  p->lw_wmax.clear();
  p->lw_bytes = 0;
  if (!pattern_tables_eligible(p)) return;
  emit_lw_records(f);
  table_depths(p);
  if (!tsim_tables_plan(p, p->lw_cap_now, p->lw_budget)) {
    p->lw_wmax.clear();
    return;
  }
  if (p->lw_wide) {
    emit_wide_records(f);
    return;
  }
  p->lw = true;
  emit_fsel_programs(f);
  emit_reg_tables(f);
  emit_fast_record(f);
  emit_fastm_record(f);
  emit_gen_record(f);
  if (p->lw_trie && !p->gr_off) {  // (only k_sample_gen walks the prefix trees)
    p->lw = false;
    p->lw_trie = false;
    p->lw_wmax.clear();
  }
}

// ---------------------------------------------------------------------------
// the end of the host stages: shadow records, tail padding, the plan line
// ---------------------------------------------------------------------------
// TSIM_AMD_DEBUG=finalize: every scalar the host stages decided, on one line beside the image hashes (the image is pinned by
// the hashes, the routing fields the launchers read by this line: tests/test_packer_image.py)
template <class It>
void plan_list(std::string &s, const char *key, It b, It e) {
  s += std::string(" ") + key + "=";
  if (b == e) s += "-";
  for (It i = b; i != e; ++i) s += (i == b ? "" : "/") + std::to_string((long long)*i);
}
void print_plan(const tsim_program *p) {
  std::string s;
  auto num = [&](const char *key, long long v) { plan_list(s, key, &v, &v + 1); };
  num("fast", p->fast), num("sampleable", p->sampleable), num("total_keys", p->total_keys), num("hw_max_rows", p->hw_max_rows);
  plan_list(s, "comp_w", p->comp_w.begin(), p->comp_w.end());
  num("v4", p->v4), num("v4w", p->v4w), num("v4_gt", p->v4_gt), num("v4_max_nch", p->v4_max_nch), num("v4_max_sent", p->v4_max_sent);
  num("wide_big", p->wide_big), num("v4w_resident_bytes", (long long)p->v4w_resident_bytes);
  num("lw", p->lw), num("lw_wide", p->lw_wide), num("lw_reg", p->lw_reg), num("lw_trie", p->lw_trie), num("narrow_big", p->narrow_big);
  std::vector<int> trie;
  for (auto &c : p->comps) trie.push_back(c.trie ? 1 : 0);
  plan_list(s, "trie", trie.begin(), trie.end());
  num("lw_cap_max", p->lw_cap_max), num("lw_cap_default", p->lw_cap_default), num("lw_cap_now", p->lw_cap_now);
  num("lw_budget", p->lw_budget), num("lw_trie_budget", p->lw_trie_budget);
  plan_list(s, "lw_wmax", p->lw_wmax.begin(), p->lw_wmax.end());
  num("lw_bytes", p->lw_bytes);
  num("direct_off", p->direct_off), num("comp_off", p->comp_off), num("comp4_off", p->comp4_off), num("lw_off", p->lw_off);
  num("lw_binom_off", p->lw_binom_off), num("lw_binom_stride", p->lw_binom_stride);
  plan_list(s, "wr_offs", p->wr_offs.begin(), p->wr_offs.end());
  num("lwf_off", p->lwf_off), num("lwfm_off", p->lwfm_off), num("gr_off", p->gr_off);
  num("lw_direct_prog", p->lw_direct_prog), num("lw_direct_chunks", p->lw_direct_chunks), num("lw_direct_rot", p->lw_direct_rot);
  num("lw_shadow_off", p->lw_shadow_off);
  plan_list(s, "stats", p->stats, p->stats + 8);
  num("defer_group", p->knobs.defer_group), num("image", (long long)p->img.size());
  fprintf(stderr, "[tsim] finalize: plan%s\n", s.c_str());
}

int finish_image(Finalize &f) {
  tsim_program *p = f.p;
  if (p->lw) {  // shadow copy of the LW records: what a table build in the background unranks from (tsim_tables.hip)
    f.w.align(32);
    p->lw_shadow_off = (int)f.w.grow(p->comps.size() * LW_WORDS);
  }
  f.w.grow(256);  // tail padding: wide scalar loads may over-read
  if (p->img.size() >= (1ull << 30)) return tsim_fail(TSIM_ENOTSUP, "program image too large");  // (4 GB: the term-table gathers use 32-bit byte offsets)
  if (p->knobs.defer_group <= 0)  // (not told by TSIM_AMD_TUNE) launches per deferred batch: a batch lasts about as long as ONE hard-row
    p->knobs.defer_group = p->stats[5] > (4ll << 20) ? 8 : 4;  // pass; 4 for small programs, 8 beyond 4 MB of chunk tables (C4)
  f.mark("pattern-table plan, first-pass records");
  if (f.dbg) print_plan(p);
  return 0;
}

// ---------------------------------------------------------------------------
// stage: upload, table build, the start of the background build
// ---------------------------------------------------------------------------
// launch-plan feedback buffer (mapped pinned host memory the hard-row kernels write)
int alloc_feedback(tsim_program *p) {
  if (p->v4 || p->lw_wide) {
    void *h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess) {
      void *d = nullptr;
      if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
        p->h_feedback = (volatile uint32_t *)h;
        p->d_feedback = (uint32_t *)d;
        for (int i = 0; i < 16; ++i) p->h_feedback[i] = 0xFFFFFFFFu;
      } else {
        (void)hipHostFree(h);
      }
    }
    (void)hipGetLastError();  // feedback is optional: without it every launch takes the default plan
  }
  return 0;
}

int upload_and_build(Finalize &f, int device) {
  tsim_program *p = f.p;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return tsim_fail(TSIM_EINVAL, "device %d out of range (%d visible)", device, ndev);
  p->device = device;
  HIP_TRY(hipSetDevice(device));
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) p->n_cu = cu;
  }
  if (int r = tsim_stream_acquire(device, p->stream_idx, &p->stream)) return r;
  HIP_TRY(hipMalloc((void **)&p->d_img, p->img.size() * 4));
  HIP_TRY(hipMemcpy(p->d_img, p->img.data(), p->img.size() * 4, hipMemcpyHostToDevice));
  // The deviation words start at zero through a BLOCKING copy, not hipMemset: a memset of device memory may still be in flight on
  // the null stream when finalize returns, the handle's streams are non-blocking, and a handle without a table build has nothing
  // in between - the first launch's check lane wrote its deviation and the memset landed on top of it (C5 on the row kernel
  // returned max_norm_dev 0 for 1.19e-07 in about one fresh handle of three).
  const std::vector<float> no_dev(std::max<size_t>(1, p->comps.size()), 0.0f);
  HIP_TRY(hipMalloc((void **)&p->d_dev, no_dev.size() * 4));
  HIP_TRY(hipMemcpy(p->d_dev, no_dev.data(), no_dev.size() * 4, hipMemcpyHostToDevice));
  f.mark("stream, image upload");
  if (p->lw) {
    if (int r = tsim_tables_build(p, nullptr)) return r;
    if (int r = alloc_feedback(p)) return r;
  }
  f.mark("pattern tables built");
  if (p->lw && p->lw_cap_now < p->lw_cap_default) {
    // the default depth, in the background - behind the handle's lanes in stream order of creation (tsim_tables.hip: ext_alloc_thread;
    // pooled streams: only the first handles of a process pay for hipStreamCreate)
    for (int k = 1; k <= 4; ++k)
      if (int r = slot_prepare(p, k, 0)) return r;
    (void)tsim_tables_extend_begin(p, p->lw_cap_default);
  }
  p->finalized = true;
  return TSIM_OK;
}

}  // namespace

extern "C" int tsim_program_finalize(tsim_program *p, int32_t device) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (p->finalized) return tsim_fail(TSIM_ESTATE, "program already finalized");
  read_knobs(p);
  Finalize f(p);
  choose_formulation(p);
  int r;
  do r = pack(f);  // (at most twice: the second run is on the faithful formulation)
  while (r == kAgainFaithful);
  if (r) return r;
  chunk_tables(f);
  direct_programs(f);
  pattern_table_plan(f);
  if (int e = finish_image(f)) return e;
  return upload_and_build(f, device);
}
