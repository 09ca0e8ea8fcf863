// tsim_program.hip - handle life cycle of the C ABI (include/tsim_hip.h): create, add, info, destroy, plus the memory /
// stream plumbing.  tsim_program_finalize (description -> packed image -> upload) is tsim_finalize.hip.  No kernels are defined here.
#include "tsim_internal.hip.h"
#include <map>

using namespace tsimk;
using namespace tsimhost;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

bool tsim_debug(const char *what) {
  const char *e = getenv("TSIM_AMD_DEBUG");
  return e && strstr(e, what) != nullptr;
}

int tsim_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

// ---------------------------------------------------------------------------
// the stream pool (tsim_internal.hip.h)
// ---------------------------------------------------------------------------
namespace {
struct PooledStream { hipStream_t s; int index; bool free; };
struct StreamPool { std::mutex m; std::map<int, std::vector<PooledStream>> all; };  // keyed by the real device id (`device & 15` aliased devices 16+)
StreamPool &stream_pool() { static StreamPool *sp = new StreamPool; return *sp; }  // (never destroyed: HIP may be gone at exit)
}  // namespace

int tsim_stream_acquire(int device, std::vector<int> &held, hipStream_t *out) {
  StreamPool &sp = stream_pool();
  std::lock_guard<std::mutex> lk(sp.m);
  auto &v = sp.all[device];
  unsigned busy_q = 0;
  for (int i : held) busy_q |= 1u << (i & 3);
  PooledStream *pick = nullptr;
  for (auto &e : v)  // a free stream on a hardware queue this handle does not use yet, else any free one
    if (e.free && !((busy_q >> (e.index & 3)) & 1u)) { pick = &e; break; }
  if (!pick && busy_q == 0xFu)
    for (auto &e : v)
      if (e.free) { pick = &e; break; }
  if (!pick) {
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    v.push_back(PooledStream{s, (int)v.size(), true});
    pick = &v.back();
  }
  pick->free = false;
  held.push_back(pick->index);
  *out = pick->s;
  return 0;
}

void tsim_stream_release(int device, hipStream_t s) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  StreamPool &sp = stream_pool();
  std::lock_guard<std::mutex> lk(sp.m);
  for (auto &e : sp.all[device])
    if (e.s == s) { e.free = true; return; }
  (void)hipStreamDestroy(s);  // not one of ours
}

extern "C" const char *tsim_last_error(void) { return g_err; }
extern "C" const char *tsim_tune_keys(void) {
  return "defer_hard,defer_group,lw_fast,wide_fused,wide_compact,wide_tables,wide_depth,wide_passes,hard_wave,hard_wave_rows,hard_inline_rows,"
         "hard_comp_par,hard_overflow,deep_after,fused_lanes,fused_max,gen,trie,shallow,x3,x4,noise_wave,noise_fused";
}
extern "C" const char *tsim_version(void) { return "tsim_amd-hip 0.2 (gfx950)"; }

int tsim_set_device(const tsim_program *p) {
  HIP_TRY(hipSetDevice(p->device));
  return 0;
}

// ---------------------------------------------------------------------------
// construction
// ---------------------------------------------------------------------------
extern "C" int tsim_program_create(int32_t num_outputs, int32_t num_detectors, int32_t n_direct,
                                   const int32_t *direct_f_indices, const uint8_t *direct_flips,
                                   const int32_t *output_order, tsim_program **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  if (num_outputs < 0 || n_direct < 0 || n_direct > num_outputs || num_detectors < 0)
    return tsim_fail(TSIM_EINVAL, "bad counts: num_outputs=%d n_direct=%d num_detectors=%d", num_outputs,
                n_direct, num_detectors);
  if (n_direct > 0 && (!direct_f_indices || !direct_flips)) return tsim_fail(TSIM_EINVAL, "direct arrays NULL");
  if (num_outputs > 0 && !output_order) return tsim_fail(TSIM_EINVAL, "output_order is NULL");
  tsim_program *p = new (std::nothrow) tsim_program();
  if (!p) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  p->num_outputs = num_outputs;
  p->num_detectors = num_detectors;
  p->n_direct = n_direct;
  p->direct_f.assign(direct_f_indices, direct_f_indices + n_direct);
  p->direct_flips.assign(direct_flips, direct_flips + n_direct);
  p->output_order.assign(output_order, output_order + num_outputs);
  std::vector<char> seen(num_outputs, 0);
  for (int i = 0; i < num_outputs; ++i) {
    int o = p->output_order[i];
    if (o < 0 || o >= num_outputs || seen[o]) {
      delete p;
      return tsim_fail(TSIM_EINVAL, "output_order is not a permutation of 0..%d", num_outputs - 1);
    }
    seen[o] = 1;
  }
  for (int i = 0; i < n_direct; ++i) {
    if (p->direct_f[i] < 0) {
      delete p;
      return tsim_fail(TSIM_EINVAL, "negative direct_f_indices[%d]", i);
    }
    p->max_f_index = std::max(p->max_f_index, p->direct_f[i]);
  }
  *out = p;
  return TSIM_OK;
}

extern "C" int tsim_program_add_component(tsim_program *p, int32_t n_out, const int32_t *output_indices,
                                          int32_t F, const int32_t *f_selection, int32_t n_levels) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (p->finalized) return tsim_fail(TSIM_ESTATE, "program already finalized");
  if (n_out < 0 || F < 0) return tsim_fail(TSIM_EINVAL, "negative n_out/F");
  if (n_levels != n_out + 1 && n_levels != 2)
    return tsim_fail(TSIM_EINVAL, "component with %d outputs needs %d (sequential) or 2 (joint) levels, got %d",
                n_out, n_out + 1, n_levels);
  if ((n_out > 0 && !output_indices) || (F > 0 && !f_selection)) return tsim_fail(TSIM_EINVAL, "NULL index array");
  HostComponent c;
  c.n_out = n_out;
  c.F = F;
  c.n_levels = n_levels;
  c.output_indices.assign(output_indices, output_indices + n_out);
  c.f_selection.assign(f_selection, f_selection + F);
  for (int i = 0; i < F; ++i) {
    if (c.f_selection[i] < 0) return tsim_fail(TSIM_EINVAL, "negative f_selection[%d]", i);
    p->max_f_index = std::max(p->max_f_index, c.f_selection[i]);
  }
  p->comps.push_back(std::move(c));
  return (int)p->comps.size() - 1;
}

template <class T>
static void copy_arr(std::vector<T> &dst, const T *src, size_t n) {
  if (n && src) dst.assign(src, src + n);
  else dst.assign(n, T());
}

extern "C" int tsim_program_add_level(tsim_program *p, int32_t component, const tsim_level_desc *L) {
  if (!p || !L) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (p->finalized) return tsim_fail(TSIM_ESTATE, "program already finalized");
  if (component < 0 || component >= (int)p->comps.size()) return tsim_fail(TSIM_EINVAL, "bad component index %d", component);
  HostComponent &c = p->comps[component];
  if ((int)c.levels.size() >= c.n_levels) return tsim_fail(TSIM_EINVAL, "component %d already has all %d levels", component, c.n_levels);
  const int k = (int)c.levels.size();
  const bool sequential = (c.n_levels == c.n_out + 1);
  const int want_P = c.F + (sequential ? k : (k == 0 ? 0 : c.n_out));
  if (L->n_params != want_P)
    return tsim_fail(TSIM_EINVAL, "component %d level %d: n_params=%d, expected %d", component, k, L->n_params, want_P);
  if (L->num_graphs < 0 || L->ta < 0 || L->tb < 0 || L->tc < 0 || L->td < 0) return tsim_fail(TSIM_EINVAL, "negative sizes");
  if (L->n_params > TSIM_MAX_PARAMS)
    return tsim_fail(TSIM_ENOTSUP, "n_params=%d exceeds TSIM_MAX_PARAMS=%d", L->n_params, TSIM_MAX_PARAMS);
  const size_t G = L->num_graphs, P = L->n_params;
  if (G > 0) {
    const void *req[] = {L->phase_indices, L->floatfactor, L->power2};
    for (const void *q : req)
      if (!q) return tsim_fail(TSIM_EINVAL, "prefactor array is NULL");
    if ((L->ta && (!L->a_phases || !L->a_counts || (P && !L->a_params))) ||
        (L->tb && (!L->b_coeffs || (P && !L->b_params))) ||
        (L->tc && (!L->c_psi_const || !L->c_phi_const || (P && (!L->c_psi_params || !L->c_phi_params)))) ||
        (L->td && (!L->d_alpha || !L->d_beta || !L->d_counts || (P && (!L->d_alpha_params || !L->d_beta_params)))))
      return tsim_fail(TSIM_EINVAL, "term array is NULL");
    if (L->has_approx && !L->approx) return tsim_fail(TSIM_EINVAL, "has_approx set but approx is NULL");
  }
  HostLevel h;
  h.G = (int)G;
  h.P = (int)P;
  h.approx = L->has_approx != 0;
  h.d = *L;
  copy_arr(h.u8[0], L->a_phases, G * L->ta);
  copy_arr(h.u8[1], L->a_params, G * L->ta * P);
  copy_arr(h.u8[2], L->b_coeffs, G * L->tb);
  copy_arr(h.u8[3], L->b_params, G * L->tb * P);
  copy_arr(h.u8[4], L->c_psi_const, G * L->tc);
  copy_arr(h.u8[5], L->c_psi_params, G * L->tc * P);
  copy_arr(h.u8[6], L->c_phi_const, G * L->tc);
  copy_arr(h.u8[7], L->c_phi_params, G * L->tc * P);
  copy_arr(h.u8[8], L->d_alpha, G * L->td);
  copy_arr(h.u8[9], L->d_alpha_params, G * L->td * P);
  copy_arr(h.u8[10], L->d_beta, G * L->td);
  copy_arr(h.u8[11], L->d_beta_params, G * L->td * P);
  copy_arr(h.u8[12], L->phase_indices, G);
  copy_arr(h.i32[0], L->a_counts, L->ta ? G : 0);
  copy_arr(h.i32[1], L->d_counts, L->td ? G : 0);
  copy_arr(h.i32[2], L->floatfactor, G * 4);
  copy_arr(h.i32[3], L->power2, G);
  if (L->approx) copy_arr(h.approx_v, L->approx, G * 2);
  else { h.approx_v.assign(G * 2, 0.0f); for (size_t g = 0; g < G; ++g) h.approx_v[2 * g] = 1.0f; }
  for (size_t g = 0; g < G; ++g) {
    if (L->ta && (h.i32[0][g] < 0 || h.i32[0][g] > L->ta)) return tsim_fail(TSIM_EINVAL, "a_counts[%zu] out of range", g);
    if (L->td && (h.i32[1][g] < 0 || h.i32[1][g] > L->td)) return tsim_fail(TSIM_EINVAL, "d_counts[%zu] out of range", g);
  }
  c.levels.push_back(std::move(h));
  return TSIM_OK;
}
extern "C" int tsim_program_set_mode(tsim_program *p, int32_t mode) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (p->finalized) return tsim_fail(TSIM_ESTATE, "program already finalized");
  if (mode != TSIM_MODE_AUTO && mode != TSIM_MODE_FAITHFUL && mode != TSIM_MODE_ROW_KERNEL)
    return tsim_fail(TSIM_EINVAL, "bad mode %d", mode);
  p->mode = mode;
  return TSIM_OK;
}
extern "C" int tsim_program_set_pattern_tables(tsim_program *p, int32_t enable, int32_t max_weight) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (p->finalized) return tsim_fail(TSIM_ESTATE, "program already finalized");
  if (enable < -1 || enable > 1 || max_weight < -1 || max_weight > TSIMK_LW_MAX_WEIGHT)
    return tsim_fail(TSIM_EINVAL, "bad pattern-table setting (%d, %d)", enable, max_weight);
  p->lw_request = enable;
  p->lw_weight_cap = max_weight;
  return TSIM_OK;
}

extern "C" int tsim_program_pattern_table_info(const tsim_program *p, int32_t *enabled, int64_t *table_bytes,
                                               int32_t *max_weight) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (!p->finalized) return tsim_fail(TSIM_ESTATE, "program not finalized");
  if (enabled) *enabled = p->lw ? 1 : 0;
  if (table_bytes) *table_bytes = p->lw ? p->lw_bytes : 0;
  if (max_weight)
    for (size_t i = 0; i < p->comps.size(); ++i) max_weight[i] = p->lw ? p->lw_wmax[i] : -1;
  return TSIM_OK;
}
extern "C" int tsim_program_tables_pending(const tsim_program *p, int32_t *pending) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (!p->finalized) return tsim_fail(TSIM_ESTATE, "program not finalized");
  if (pending) *pending = p->ext_pending ? 1 : 0;
  return TSIM_OK;
}
extern "C" void tsim_program_destroy(tsim_program *p) {
  if (!p) return;
  if (p->device >= 0) (void)hipSetDevice(p->device);
  for (hipStream_t &a : p->aux)
    if (a) { tsim_stream_release(p->device, a); a = nullptr; }
  if (p->finalized && p->device >= 0) {
    (void)hipSetDevice(p->device);
    (void)tsim_flush_hard(p);  // parked hard rows of launches that were never joined: finish them, then drain every lane
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (auto &sl : p->slots)
      if (sl.side_ready) (void)hipStreamSynchronize(sl.side);
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    if (tsim_debug("pipeline"))
      fprintf(stderr, "tsim pipeline: begins %llu deferred %llu flushes %llu queries %llu waits %llu fused groups %llu (specialised %llu, component-parallel hard rows %llu)\n",
              p->stat_begins, p->stat_deferred, p->stat_flushes, p->stat_queries, p->stat_waits, p->stat_fused, p->stat_fast, p->stat_partial);
    if (p->sync_ev) (void)hipEventDestroy(p->sync_ev);
    for (hipEvent_t e : p->lane_ev) if (e) (void)hipEventDestroy(e);
    for (auto &cs : p->caller_streams) if (cs.ev) (void)hipEventDestroy(cs.ev);
    for (hipEvent_t e : p->over_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->batch_ev) if (e) (void)hipEventDestroy(e);
    for (void *s : p->scratch)
      if (s) (void)hipFree(s);
    for (void *q : p->owned) (void)hipFree(q);  // buffers the caller never returned
    p->owned.clear();
    p->ext_abort.store(true, std::memory_order_release);
    if (p->ext_thread.joinable()) p->ext_thread.join();
    if (p->ext_stream) tsim_stream_release(p->device, p->ext_stream);
    // a table build in the background: its slices ran on whatever stream the next launch used - the lanes drained above, but
    // tsim_sample_batch_device puts them on CALLER streams too, which the handle cannot drain one by one
    if (p->ext_pending) (void)hipDeviceSynchronize();
    if (p->d_img) (void)hipFree(p->d_img);
    if (p->d_dev) (void)hipFree(p->d_dev);
    for (void *q : p->ext_scratch) (void)hipFree(q);
    if (p->ext_tab) (void)hipFree(p->ext_tab);
    if (p->ext_ev) (void)hipEventDestroy(p->ext_ev);
    if (p->d_lw_tab) (void)hipFree(p->d_lw_tab);
    if (p->ctl_block) (void)hipFree(p->ctl_block);  // (the slots' counter sets: one allocation)
    if (p->h_feedback) (void)hipHostFree((void *)p->h_feedback);
    for (auto &sl : p->slots) {
      if (sl.hard) (void)hipFree(sl.hard);
      if (sl.hard2) (void)hipFree(sl.hard2);
      if (sl.keys) (void)hipFree(sl.keys);
      if (sl.ev1) (void)hipEventDestroy(sl.ev1);
      if (sl.ev2) (void)hipEventDestroy(sl.ev2);

      if (sl.side && !sl.side_borrowed) tsim_stream_release(p->device, sl.side);
    }
    if (p->stream) tsim_stream_release(p->device, p->stream);
  } else if (p->device >= 0) {
    // a finalize that failed after it had taken streams / device memory (the pooled streams stayed marked busy for good)
    if (p->ext_thread.joinable()) { p->ext_abort.store(true, std::memory_order_release); p->ext_thread.join(); }
    if (p->ext_stream) tsim_stream_release(p->device, p->ext_stream);
    for (auto &sl : p->slots)
      if (sl.side && !sl.side_borrowed) tsim_stream_release(p->device, sl.side);
    if (p->stream) tsim_stream_release(p->device, p->stream);
    if (p->d_img) (void)hipFree(p->d_img);
    if (p->d_dev) (void)hipFree(p->d_dev);
    if (p->d_lw_tab) (void)hipFree(p->d_lw_tab);
    if (p->h_feedback) (void)hipHostFree((void *)p->h_feedback);
    (void)hipGetLastError();
  }
  delete p;
}

extern "C" int tsim_program_stats(const tsim_program *p, int64_t out[8]) {
  if (!p || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!p->finalized) return tsim_fail(TSIM_ESTATE, "program not finalized");
  for (int i = 0; i < 8; ++i) out[i] = p->stats[i];
  out[0] = p->fast ? 1 : 0;
  return TSIM_OK;
}

extern "C" int tsim_program_path_counts(tsim_program *p, int64_t out[TSIM_PATH_COUNT], int32_t reset) {
  if (!p || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  for (int i = 0; i < TSIM_PATH_COUNT; ++i) {
    out[i] = p->path_count[i];
    if (reset) p->path_count[i] = 0;
  }
  return TSIM_OK;
}

extern "C" int tsim_program_get_mode(const tsim_program *p, int32_t *fast) {
  if (!p || !fast) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!p->finalized) return tsim_fail(TSIM_ESTATE, "program not finalized");
  *fast = p->fast ? 1 : 0;
  return TSIM_OK;
}

extern "C" int tsim_program_info(const tsim_program *p, int32_t *n_components, int32_t *num_outputs,
                                 int64_t *image_bytes, int64_t *total_graphs, int64_t *total_rows) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (n_components) *n_components = (int32_t)p->comps.size();
  if (num_outputs) *num_outputs = p->num_outputs;
  if (image_bytes) *image_bytes = (int64_t)p->img.size() * 4;
  if (total_graphs) *total_graphs = p->total_graphs;
  if (total_rows) *total_rows = p->total_rows;
  return TSIM_OK;
}
int tsim_need_final(const tsim_program *p) {
  if (!p) return tsim_fail(TSIM_EINVAL, "program is NULL");
  if (!p->finalized) return tsim_fail(TSIM_ESTATE, "program not finalized");
  return 0;
}

int tsim_ensure_scratch(tsim_program *p, int slot, size_t bytes) {
  if (p->scratch_sz[slot] >= bytes) return 0;
  if (p->scratch[slot]) {
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipFree(p->scratch[slot]));
    p->scratch[slot] = nullptr;
    p->scratch_sz[slot] = 0;
  }
  size_t cap = std::max<size_t>(bytes, 256);
  hipError_t e = hipMalloc(&p->scratch[slot], cap);
  if (e != hipSuccess) return tsim_fail(TSIM_ENOMEM, "hipMalloc(%zu) failed: %s", cap, hipGetErrorString(e));
  p->scratch_sz[slot] = cap;
  return 0;
}
// ---------------------------------------------------------------------------
// plumbing
// ---------------------------------------------------------------------------
extern "C" int tsim_device_count(int32_t *count) {
  if (!count) return tsim_fail(TSIM_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return tsim_fail(TSIM_EHIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  }
  *count = n;
  return TSIM_OK;
}

extern "C" int tsim_malloc_device(tsim_program *p, int64_t nbytes, void **d_ptr) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (!d_ptr || nbytes < 0) return tsim_fail(TSIM_EINVAL, "bad argument");
  hipError_t e = hipMalloc(d_ptr, (size_t)std::max<int64_t>(nbytes, 1));
  if (e != hipSuccess) return tsim_fail(TSIM_ENOMEM, "hipMalloc(%lld) failed: %s", (long long)nbytes, hipGetErrorString(e));
  p->owned.insert(*d_ptr);
  return TSIM_OK;
}

extern "C" int tsim_free_device(tsim_program *p, void *d_ptr) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (!d_ptr) return TSIM_OK;
  if (!p->owned.erase(d_ptr)) return tsim_fail(TSIM_EINVAL, "pointer was not allocated by tsim_malloc_device on this handle");
  HIP_TRY(hipFree(d_ptr));
  return TSIM_OK;
}

extern "C" int tsim_mem_info(tsim_program *p, int64_t *free_bytes, int64_t *total_bytes) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  size_t f = 0, t = 0;
  HIP_TRY(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return TSIM_OK;
}

extern "C" int tsim_malloc_pinned(int64_t nbytes, void **h_ptr) {
  if (!h_ptr || nbytes < 0) return tsim_fail(TSIM_EINVAL, "bad argument");
  hipError_t e = hipHostMalloc(h_ptr, (size_t)std::max<int64_t>(nbytes, 1), hipHostMallocDefault);
  if (e != hipSuccess) return tsim_fail(TSIM_ENOMEM, "hipHostMalloc(%lld) failed: %s", (long long)nbytes, hipGetErrorString(e));
  return TSIM_OK;
}

extern "C" int tsim_free_pinned(void *h_ptr) {
  HIP_TRY(hipHostFree(h_ptr));
  return TSIM_OK;
}

extern "C" int tsim_memcpy_h2d(tsim_program *p, void *d_dst, const void *h_src, int64_t nbytes) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (nbytes < 0) return tsim_fail(TSIM_EINVAL, "negative size");
  if (nbytes == 0) return TSIM_OK;
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, (size_t)nbytes, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return TSIM_OK;
}

extern "C" int tsim_memcpy_d2h(tsim_program *p, void *h_dst, const void *d_src, int64_t nbytes) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (nbytes < 0) return tsim_fail(TSIM_EINVAL, "negative size");
  if (nbytes == 0) return TSIM_OK;
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)nbytes, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return TSIM_OK;
}

// Asynchronous copies on a caller-chosen stream (e.g. an auxiliary stream of the handle): the end-to-end sampler moves
// finished batches to the host while later ones are still being sampled (utils/cuda_helpers.py:105-141 copies once, at
// the end).  Pageable host memory is allowed (the runtime stages it; the call may then block until the copy is done).
extern "C" int tsim_memcpy_d2h_async(tsim_program *p, void *h_dst, const void *d_src, int64_t nbytes, void *stream) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (nbytes < 0) return tsim_fail(TSIM_EINVAL, "negative size");
  if (nbytes == 0) return TSIM_OK;
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)nbytes, hipMemcpyDeviceToHost, stream ? (hipStream_t)stream : p->stream));
  return TSIM_OK;
}

extern "C" int tsim_memcpy_h2d_async(tsim_program *p, void *d_dst, const void *h_src, int64_t nbytes, void *stream) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (nbytes < 0) return tsim_fail(TSIM_EINVAL, "negative size");
  if (nbytes == 0) return TSIM_OK;
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, (size_t)nbytes, hipMemcpyHostToDevice, stream ? (hipStream_t)stream : p->stream));
  return TSIM_OK;
}

extern "C" int tsim_stream_synchronize(tsim_program *p, void *stream) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  HIP_TRY(hipStreamSynchronize(stream ? (hipStream_t)stream : p->stream));
  return TSIM_OK;
}

// Auxiliary streams owned by the handle (index 0 .. TSIM_AUX_STREAMS-1, created on first use, destroyed with it): for
// work beside the sampling lanes - the device-side channel sampler, host transfers.
extern "C" int tsim_aux_stream(tsim_program *p, int32_t index, void **stream) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (index < 0 || index >= TSIM_AUX_STREAMS || !stream) return tsim_fail(TSIM_EINVAL, "bad auxiliary stream %d", index);
  if (!p->aux[index])
    if (int r = tsim_stream_acquire(p->device, p->stream_idx, &p->aux[index])) return r;
  *stream = (void *)p->aux[index];
  return TSIM_OK;
}

// The pipeline slot the next batch of tsim_sample_steps_device will use (its rotation over all TSIM_PIPELINE_SLOTS):
// what a caller needs to join exactly that batch later (tsim_sample_batch_device_end on the slot).
extern "C" int tsim_pipeline_next_slot(tsim_program *p, int32_t *slot) {
  if (int r = tsim_need_final(p)) return r;
  if (!slot) return tsim_fail(TSIM_EINVAL, "NULL argument");
  *slot = (int32_t)(p->steps_slot % (unsigned long long)TSIM_PIPELINE_SLOTS);
  return TSIM_OK;
}

extern "C" int tsim_get_stream(tsim_program *p, void **stream) {
  if (int r = tsim_need_final(p)) return r;
  if (!stream) return tsim_fail(TSIM_EINVAL, "stream is NULL");
  *stream = (void *)p->stream;
  return TSIM_OK;
}

extern "C" void tsim_key_split(uint32_t key_hi, uint32_t key_lo, uint32_t out[4]) {
  // new_key, subkey = jax.random.split(key) (threefry_partitionable): counters (0,0) and (0,1)
  uint32_t a0 = 0u, a1 = 0u, b0 = 0u, b1 = 1u;
  threefry2x32(key_hi, key_lo, a0, a1);
  threefry2x32(key_hi, key_lo, b0, b1);
  out[0] = a0; out[1] = a1; out[2] = b0; out[3] = b1;
}

extern "C" int tsim_sample_batch_device_begin_split(tsim_program *p, int32_t slot, const uint64_t *d_f, int64_t B,
                                                    int32_t num_f, uint32_t key[2], int64_t shot_offset, uint64_t *d_out,
                                                    float *d_max_norm_dev, void *stream, uint32_t flags) {
  if (!key) return tsim_fail(TSIM_EINVAL, "key is NULL");
  uint32_t o[4];
  tsim_key_split(key[0], key[1], o);  // key, subkey = split(key)  (sampler.py:399)
  key[0] = o[0];
  key[1] = o[1];
  return tsim_sample_batch_device_begin(p, slot, d_f, B, num_f, o[2], o[3], shot_offset, d_out, d_max_norm_dev, stream,
                                        flags);
}

extern "C" int tsim_synchronize(tsim_program *p) {
  if (int r = tsim_need_final(p)) return r;
  if (int r = tsim_set_device(p)) return r;
  if (int r = tsim_flush_hard(p)) return r;
  HIP_TRY(hipStreamSynchronize(p->stream));
  // the four lanes of the deferred plan (two of first passes, two of hard-row batches) and every slot stream a launch actually ran on (a stream that never
  // carried work has nothing to wait for - and each hipStreamSynchronize costs a few microseconds)
  for (int k = 1; k <= TSIM_PIPELINE_SLOTS; ++k) {
    tsim_program::Slot &sl = p->slots[k];
    if (!sl.side_ready) continue;
    if ((k <= 4 || sl.used) && sl.side != p->stream) HIP_TRY(hipStreamSynchronize(sl.side));
    sl.pending = false;
  }
  return TSIM_OK;
}
