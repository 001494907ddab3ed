// mpcqp_fleet.hip -- device-resident closed loop for a fleet of vehicles.
//
// One mpcqp_fleet_step = for every RUNNING vehicle, one iteration of the loop body of
// TrajectoryTracker.track (src/pipeline/control_stage.py:100-150):
//   k_fleet_build(relax=0)  window gather + tail padding (:101-105) fused into K1; mask = RUNNING
//   K2 (nominal ws)         _solve_with_relaxation's first solve (:43-46)
//   k_fleet_build(relax=1)  vehicles whose nominal status is not solved/solved_inaccurate
//                           (mpc_controller.py:137-139) get the relaxed window (v * 0.6, :48-49)
//   K2 (relaxed ws)         the retry with widened du_bounds (:50-56), masked to those vehicles
//   k_fleet_advance         abort (:108-110), plant f_discrete (:127), u_prev (:129),
//                           path_idx advance (:141-145), goal test (:147-150), trace (:128)
// The window is never materialised: lane k of a vehicle's wave reads row
// min(path_idx + k, len - 1) of its reference, which is numpy's slice + np.repeat padding.
#include "mpcqp_build.h"

namespace {
using mpcqp::fail;
using mpcqp::Launch;

__global__ __launch_bounds__(kWave) void k_fleet_build(mpcqp_params p, mpcqp_fleet f, int relax,
                                                       double* __restrict__ model) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int V = f.vehicles;
  if (b >= V) return;
  bool go;
  if (relax) {
    const int st = f.status[b];
    go = f.mask[b] && !(st == MPCQP_SOLVED || st == MPCQP_SOLVED_INACCURATE);
  } else {
    go = f.phase[b] == MPCQP_FLEET_RUNNING;
    // device-side validation of the loop state a C-ABI caller hands over (check_fleet cannot see
    // device data): an unusable reference aborts the vehicle, a full trace ends its run -- before
    // any indexed access
    const int len0 = f.ref_len[b], pi0 = f.path_idx[b], st0 = f.steps[b];
    const bool bad_ref = len0 < 1 || len0 > f.ref_stride || pi0 < 0;
    const bool full = st0 < 0 || st0 >= f.max_steps;
    if (go && (bad_ref || full)) {
      if (lane == 0) f.phase[b] = bad_ref ? MPCQP_FLEET_ABORTED : MPCQP_FLEET_OUT_OF_STEPS;
      go = false;
    }
  }
  if (lane == 0) f.mask[(size_t)relax * V + b] = go ? 1 : 0;
  if (!go) return;
  const int N = p.horizon;
  const int len = f.ref_len[b];
  const int pidx = f.path_idx[b];
  const double x0l = lane < 4 ? f.state[(size_t)b * 4 + lane] : 0.0;
  const double upl = (lane >= 4 && lane < 6) ? f.u_prev[(size_t)b * 2 + lane - 4] : 0.0;
  // window row k = ref[min(path_idx + k, len - 1)] (tail padding, control_stage.py:101-105)
  auto fetch = [&](int k, double& rx, double& ry, double& ryaw, double& rv) {
    const double* r = f.ref_global + ((size_t)b * f.ref_stride + min(pidx + k, len - 1)) * 4;
    rx = r[0];
    ry = r[1];
    ryaw = r[2];
    rv = relax ? r[3] * 0.6 : r[3];  // relaxed_reference[:, 3] *= 0.6 (control_stage.py:48-49)
  };
  if (N + 1 > kWave) {  // long windows: chunks of 64 rows
    build_qp_long(p, lane, fetch, x0l, upl, model + (size_t)b * model_stride(N));
    return;
  }
  double rx = 0.0, ry = 0.0, ryaw = 0.0, rv = 0.0;
  if (lane <= N) fetch(lane, rx, ry, ryaw, rv);
  build_qp(p, lane, rx, ry, ryaw, rv, x0l, upl, model + (size_t)b * model_stride(N));
}

__global__ __launch_bounds__(kWave) void k_fleet_advance(double dt, double L, mpcqp_fleet f) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * kWave + threadIdx.x;
  const int V = f.vehicles;
  if (b >= V || f.phase[b] != MPCQP_FLEET_RUNNING) return;
  int which = -1;
  const int s0 = f.status[b];
  if (s0 == MPCQP_SOLVED || s0 == MPCQP_SOLVED_INACCURATE) {
    which = 0;
  } else if (f.mask[(size_t)V + b]) {
    const int s1 = f.status[(size_t)V + b];
    if (s1 == MPCQP_SOLVED || s1 == MPCQP_SOLVED_INACCURATE) which = 1;
  }
  if (which < 0) {
    f.phase[b] = MPCQP_FLEET_ABORTED;  // control_stage.py:108-110
    return;
  }
  const double* u = f.u0 + ((size_t)which * V + b) * 2;
  const double a = u[0], delta = u[1];
  double x[4], xn[4];
  for (int i = 0; i < 4; ++i) x[i] = f.state[(size_t)b * 4 + i];
  plant(x, a, delta, dt, L, xn);
  const int k = f.steps[b];
  if (k < 0 || k >= f.max_steps) {  // k_fleet_build already ended such a run; never write past the trace
    f.phase[b] = MPCQP_FLEET_OUT_OF_STEPS;
    return;
  }
  for (int i = 0; i < 4; ++i) f.state[(size_t)b * 4 + i] = xn[i];
  if (f.trace)
    for (int i = 0; i < 4; ++i) f.trace[((size_t)b * f.max_steps + k) * 4 + i] = xn[i];
  if (f.u_trace) {
    f.u_trace[((size_t)b * f.max_steps + k) * 2 + 0] = a;
    f.u_trace[((size_t)b * f.max_steps + k) * 2 + 1] = delta;
  }
  f.u_prev[(size_t)b * 2 + 0] = a;
  f.u_prev[(size_t)b * 2 + 1] = delta;
  f.steps[b] = k + 1;
  const int len = f.ref_len[b];
  int pi = f.path_idx[b];
  if (pi < len - 2 && fleet_off_row(xn[0], xn[1], f.ref_global + ((size_t)b * f.ref_stride + pi) * 4))
    f.path_idx[b] = pi + 1;
  int ph = MPCQP_FLEET_RUNNING;
  if (fleet_at_goal(xn[0], xn[1], f.goal[(size_t)b * 2], f.goal[(size_t)b * 2 + 1]))
    ph = MPCQP_FLEET_GOAL;
  else if (k + 1 >= f.max_steps)
    ph = MPCQP_FLEET_OUT_OF_STEPS;
  f.phase[b] = ph;
}

// the parameter blocks of one mpcqp_fleet_loop call, stream-ordered before the loop kernel
__global__ __launch_bounds__(kWave) void k_store_params(mpcqp_params pn, mpcqp_params pr, mpcqp_params* __restrict__ P) {
  static_assert(sizeof(mpcqp_params) % 4 == 0, "params copied by words");
  constexpr int W = (int)(sizeof(mpcqp_params) / 4);
  for (int w = threadIdx.x; w < W; w += kWave) {
    reinterpret_cast<uint32_t*>(P)[w] = reinterpret_cast<const uint32_t*>(&pn)[w];
    reinterpret_cast<uint32_t*>(P + 1)[w] = reinterpret_cast<const uint32_t*>(&pr)[w];
  }
}

// the 2 K blocks of one mpcqp_fleet_loop_mixed call, T = {nominal[0], relaxed[0], nominal[1], ...}, from
// the two workspaces' class tables (workgroup c copies class c), stream-ordered before the loop kernel
__global__ __launch_bounds__(kWave) void k_store_classes(const mpcqp_params* __restrict__ nom,
                                                         const mpcqp_params* __restrict__ rel, int K,
                                                         mpcqp_params* __restrict__ T) {
  constexpr int W = (int)(sizeof(mpcqp_params) / 4);
  const int c = blockIdx.x;
  if (c >= K) return;
  for (int w = threadIdx.x; w < W; w += kWave) {
    reinterpret_cast<uint32_t*>(T + 2 * (size_t)c)[w] = reinterpret_cast<const uint32_t*>(nom + c)[w];
    reinterpret_cast<uint32_t*>(T + 2 * (size_t)c + 1)[w] = reinterpret_cast<const uint32_t*>(rel + c)[w];
  }
}

// The fused loop's dispatch order: the vehicles by reference length, longest first (a bucket sort
// on the length, 1024 buckets; the order inside a bucket is immaterial -- vehicles are independent).
// One 1024-thread workgroup.
constexpr int kOrderBuckets = 1024;
__global__ __launch_bounds__(kOrderBuckets) void k_fleet_order(mpcqp_fleet f, int32_t* __restrict__ order) {
  __shared__ int cnt[kOrderBuckets];
  const int t = threadIdx.x, V = f.vehicles;
  const int span = f.ref_stride + 1;
  auto bucket = [&](int v) {
    int len = f.ref_len[v];
    len = len < 0 ? 0 : (len > f.ref_stride ? f.ref_stride : len);
    return (int)(((long long)(f.ref_stride - len) * kOrderBuckets) / span);  // longest -> bucket 0
  };
  cnt[t] = 0;
  __syncthreads();
  for (int v = t; v < V; v += kOrderBuckets) atomicAdd(&cnt[bucket(v)], 1);
  __syncthreads();
  for (int d = 1; d < kOrderBuckets; d <<= 1) {  // inclusive scan (Hillis-Steele)
    const int add = t >= d ? cnt[t - d] : 0;
    __syncthreads();
    cnt[t] += add;
    __syncthreads();
  }
  const int excl = t ? cnt[t - 1] : 0;
  __syncthreads();
  cnt[t] = excl;
  __syncthreads();
  for (int v = t; v < V; v += kOrderBuckets) order[atomicAdd(&cnt[bucket(v)], 1)] = v;
}

// mpcqp_class_slots: the two members of each wave of a class-paired mixed launch (k_solve_pair_mixed,
// k_fleet_loop_pair_mixed).  Bucket k < K holds the entries of class k, bucket K those whose class lies
// outside [0, K) (and entries outside [0, V), whose class is not read); bucket k owns the waves
// [base_k, base_k + (cnt_k + 1) / 2), base the running sum over the buckets before it, and its members
// fill those waves' slots in the order of the sequence, chunk by chunk (within a chunk of 1024 entries
// the cursor's atomics decide; the members are independent, k_fleet_order's argument).  The odd slot of a
// bucket and the waves past the used ones are written -1 by the threads that know them, so every entry of
// the table is written exactly once.  One 1024-thread workgroup: a counter per bucket in LDS (kSlotBuckets
// = MPCQP_CLASS_SLOT_MAX_CLASSES + 1, kSlotRun consecutive ones per thread) and a scan over the threads'
// sums.
constexpr int kSlotThreads = 1024;
constexpr int kSlotBuckets = MPCQP_CLASS_SLOT_MAX_CLASSES + 1;
constexpr int kSlotRun = kSlotBuckets / kSlotThreads;
static_assert(kSlotRun * kSlotThreads == kSlotBuckets, "a whole number of buckets per thread");
__global__ __launch_bounds__(kSlotThreads) void k_class_slots(int V, int K, int W, const int32_t* __restrict__ cls,
                                                              const int32_t* __restrict__ seq,
                                                              int32_t* __restrict__ slots) {
  __shared__ int cnt[kSlotBuckets];  // members per bucket, then the bucket's slot cursor
  __shared__ int part[kSlotThreads];
  const int t = threadIdx.x;
  auto member = [&](int i) { return seq ? seq[i] : i; };
  auto bucket = [&](int v) {
    if (v < 0 || v >= V) return K;
    const int c = cls[v];
    return (unsigned)c < (unsigned)K ? c : K;
  };
  for (int k = t; k < kSlotBuckets; k += kSlotThreads) cnt[k] = 0;
  __syncthreads();
  for (int i = t; i < V; i += kSlotThreads) atomicAdd(&cnt[bucket(member(i))], 1);
  __syncthreads();
  // waves per bucket, summed over this thread's run (buckets past K are empty), scanned over the threads
  int own = 0;
  for (int j = 0; j < kSlotRun; ++j) own += (cnt[t * kSlotRun + j] + 1) >> 1;
  part[t] = own;
  __syncthreads();
  for (int d = 1; d < kSlotThreads; d <<= 1) {  // inclusive scan (Hillis-Steele)
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int base = part[t] - own;  // the first wave of this thread's run
  const int used = part[kSlotThreads - 1];
  for (int j = 0; j < kSlotRun; ++j) {
    const int k = t * kSlotRun + j, n = cnt[k];
    if (n & 1) slots[2 * base + n] = -1;  // the bucket's empty half
    cnt[k] = 2 * base;
    base += (n + 1) >> 1;
  }
  for (int i = 2 * used + t; i < 2 * W; i += kSlotThreads) slots[i] = -1;  // the grid past the used waves
  __syncthreads();
  for (int i0 = 0; i0 < V; i0 += kSlotThreads) {  // a chunk at a time: its members stay ahead of the next chunk's
    const int i = i0 + t;
    if (i < V) {
      const int v = member(i);
      slots[atomicAdd(&cnt[bucket(v)], 1)] = v;
    }
    __syncthreads();
  }
}

int check_fleet(const mpcqp_ws* nom, const mpcqp_ws* rel, const mpcqp_fleet* f) {
  if (!nom || !rel || !f) return fail(MPCQP_E_ARG, "null argument");
  if (nom == rel) return fail(MPCQP_E_ARG, "nominal and relaxed workspaces must differ");
  if (nom->p.horizon != rel->p.horizon) return fail(MPCQP_E_HORIZON, "workspaces differ in horizon");
  if (nom->device != rel->device) return fail(MPCQP_E_ARG, "workspaces on different devices");
  if (f->vehicles < 0 || f->vehicles > nom->max_batch || f->vehicles > rel->max_batch)
    return fail(MPCQP_E_BATCH, "fleet exceeds workspace capacity");
  if (f->ref_stride < 1 || f->max_steps < 1) return fail(MPCQP_E_ARG, "ref_stride and max_steps must be >= 1");
  if (!f->ref_global || !f->ref_len || !f->goal || !f->state || !f->u_prev || !f->path_idx || !f->phase ||
      !f->steps || !f->mask || !f->status || !f->u0)
    return fail(MPCQP_E_ARG, "null fleet buffer");
  return MPCQP_OK;
}

// enqueue one step (no validation)
int enqueue_step(mpcqp_ws* nom, mpcqp_ws* rel, const mpcqp_fleet* f, hipStream_t s) {
  const int V = f->vehicles;
  const mpcqp::launcher_t solve = mpcqp::launcher(nom->p);
  if (mpcqp::launcher(rel->p) != solve) return fail(MPCQP_E_ARG, "nominal and relaxed workspaces differ in kernel");
  if (!solve) return fail(MPCQP_E_HORIZON, "horizon not compiled into this build");
  const int rc = mpcqp::fleet_buffers(nom, rel, s);
  if (rc) return rc;
  nom->invalidate();  // the fleet overwrites the models: a later mpcqp_solve needs its own build
  rel->invalidate();
  hipLaunchKernelGGL(k_fleet_build, dim3(V), dim3(kWave), 0, s, nom->p, *f, 0, nom->model);
  solve(s, Launch{&nom->p, V, nom->model, nom->state, f->u0, f->X, nullptr, f->status, nullptr, nullptr, f->mask});
  hipLaunchKernelGGL(k_fleet_build, dim3(V), dim3(kWave), 0, s, rel->p, *f, 1, rel->model);
  solve(s, Launch{&rel->p, V, rel->model, rel->state, f->u0 + (size_t)2 * V, f->X, nullptr, f->status + V, nullptr,
                  nullptr, f->mask + V});
  hipLaunchKernelGGL(k_fleet_advance, dim3((V + kWave - 1) / kWave), dim3(kWave), 0, s, nom->p.dt,
                     nom->p.wheelbase_px, *f);
  return mpcqp::launched("fleet step");
}

// One captured step, replayed `steps` times on a private stream ordered against the caller's.
int run_graph(mpcqp_ws* nom, mpcqp_ws* rel, const mpcqp_fleet* f, int steps, hipStream_t user) {
  return mpcqp::replay_graph(
      "fleet", user, steps, [&] { return mpcqp::fleet_buffers(nom, rel, user); },
      [&](hipStream_t s2) { return enqueue_step(nom, rel, f, s2); });
}

}  // namespace

extern "C" {

int mpcqp_class_slot_waves(int V, int K) { return mpcqp::class_slot_waves(V, K); }

int mpcqp_class_slots(int V, int K, const int32_t* cls, const int32_t* seq, int32_t* slots, void* stream) {
  if (V < 0 || !cls || !slots) return fail(MPCQP_E_ARG, "mpcqp_class_slots needs V >= 0, cls and slots");
  if (K < 1 || K > MPCQP_CLASS_SLOT_MAX_CLASSES)
    return fail(MPCQP_E_ARG, "mpcqp_class_slots: K outside [1, " + std::to_string(MPCQP_CLASS_SLOT_MAX_CLASSES) + "]");
  if (V == 0) return MPCQP_OK;
  mpcqp::enqueue_class_slots(V, K, cls, seq, slots, static_cast<hipStream_t>(stream));
  return mpcqp::launched("k_class_slots");
}

int mpcqp_fleet_step(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, void* stream) {
  int rc = check_fleet(nominal, relaxed, f);
  if (rc) return rc;
  if (f->vehicles == 0) return MPCQP_OK;
  return enqueue_step(nominal, relaxed, f, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace mpcqp {
void enqueue_class_slots(int V, int K, const int32_t* cls, const int32_t* seq, int32_t* slots, hipStream_t s) {
  hipLaunchKernelGGL(k_class_slots, dim3(1), dim3(kSlotThreads), 0, s, V, K, class_slot_waves(V, K), cls, seq,
                     slots);
}

int fleet_buffers(mpcqp_ws* nominal, mpcqp_ws* relaxed, hipStream_t s) {
  int rc = ensure_buffers(nominal, true, needs_state(nominal->p), s);
  if (rc == MPCQP_OK) rc = ensure_buffers(relaxed, true, needs_state(relaxed->p), s);
  return rc;
}

int replay_graph(const char* what, hipStream_t user, int steps, const std::function<int()>& prepare,
                 const std::function<int(hipStream_t)>& step) {
  hipStream_t s2 = nullptr;
  hipEvent_t ev = nullptr;
  hipGraph_t g = nullptr;
  hipGraphExec_t ex = nullptr;
  int rc = MPCQP_OK;
  auto cleanup = [&]() {
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
    if (ev) (void)hipEventDestroy(ev);
    if (s2) (void)hipStreamDestroy(s2);
  };
  hipError_t e = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ev, user);
  if (e == hipSuccess) e = hipStreamWaitEvent(s2, ev, 0);
  if (e == hipSuccess && (rc = prepare()) != MPCQP_OK) {  // outside the capture
    cleanup();
    return rc;
  }
  if (e == hipSuccess) e = hipStreamBeginCapture(s2, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    cleanup();
    return fail(MPCQP_E_HIP, std::string(what) + " graph setup: " + hipGetErrorString(e));
  }
  rc = step(s2);
  e = hipStreamEndCapture(s2, &g);
  if (rc == MPCQP_OK && e != hipSuccess) rc = fail(MPCQP_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  if (rc == MPCQP_OK) {
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    for (int i = 0; e == hipSuccess && i < steps; ++i) e = hipGraphLaunch(ex, s2);
    if (e == hipSuccess) e = hipEventRecord(ev, s2);
    if (e == hipSuccess) e = hipStreamWaitEvent(user, ev, 0);
    // the replays must finish before the graph and its stream are released
    if (e == hipSuccess) e = hipStreamSynchronize(s2);
    if (e != hipSuccess) rc = fail(MPCQP_E_HIP, std::string(what) + " graph replay: " + hipGetErrorString(e));
  }
  cleanup();
  return rc;
}

fleet_loop_t fused_loop(const mpcqp_ws* nominal, const mpcqp_ws* relaxed, fleet_loop_t HorizonKernels::*which) {
  const HorizonKernels *kn = one_wave(nominal->p), *kr = one_wave(relaxed->p);
  return kn && kr && kn->*which == kr->*which ? kn->*which : nullptr;
}

int check_loop_classes(const mpcqp_ws* nominal, const mpcqp_ws* relaxed, const char* who) {
  const std::string w(who);
  const int K = nominal->n_classes;
  if (K < 1 || !nominal->dclasses)
    return fail(MPCQP_E_STATE, w + ": the nominal workspace holds no class table (mpcqp_set_classes)");
  if (relaxed->n_classes < 1 || !relaxed->dclasses)
    return fail(MPCQP_E_STATE, w + ": the relaxed workspace holds no class table (mpcqp_set_classes)");
  if (relaxed->n_classes != K)
    return fail(MPCQP_E_STATE, w + ": the relaxed workspace holds " + std::to_string(relaxed->n_classes) +
                                   " classes, the nominal workspace " + std::to_string(K));
  return MPCQP_OK;
}

int grow_loop_classes(mpcqp_ws* nominal, hipStream_t s) {
  const int K = nominal->n_classes;
  if (nominal->dloop_cap >= K) return MPCQP_OK;
  // the interleaved table grows outside any capture (hipFree waits for its readers)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return fail(MPCQP_E_STATE, "the mixed loop's class table is allocated at its first use, which cannot be inside "
                               "a stream capture: run the call once uncaptured first");
  const DeviceGuard dev(nominal->device);
  hipError_t e = dev.err;
  mpcqp_params* table = nullptr;
  if (e == hipSuccess) e = hipMalloc(&table, 2 * sizeof(mpcqp_params) * (size_t)K);
  if (e != hipSuccess) return fail(MPCQP_E_HIP, std::string("hipMalloc (mixed loop classes): ") + hipGetErrorString(e));
  if (nominal->dloop_classes) (void)hipFree(nominal->dloop_classes);
  nominal->dloop_classes = table;
  nominal->dloop_cap = K;
  return MPCQP_OK;
}

int enqueue_fused_loop(mpcqp_ws* nominal, mpcqp_ws* relaxed, fleet_loop_t loop, const char* name, int kind,
                       bool may_pair, LoopLaunch L, hipStream_t s) {
  nominal->invalidate();  // as mpcqp_fleet_step: a later mpcqp_solve needs its own build
  relaxed->invalidate();
  if (L.cls) {
    L.P = nominal->dloop_classes;
    hipLaunchKernelGGL(k_store_classes, dim3(L.K), dim3(kWave), 0, s, nominal->dclasses, relaxed->dclasses, L.K,
                       nominal->dloop_classes);
  } else {
    L.P = nominal->dparams;
    hipLaunchKernelGGL(k_store_params, dim3(1), dim3(kWave), 0, s, nominal->p, relaxed->p, nominal->dparams);
  }
  // longest first only when the vehicles outnumber the wave slots (2 per SIMD): with every vehicle
  // resident at once the order only changes which vehicles share a SIMD (measured: no gain)
  if (nominal->cus > 0 && L.f->vehicles > 8 * nominal->cus) {
    hipLaunchKernelGGL(k_fleet_order, dim3(1), dim3(kOrderBuckets), 0, s, *L.f, nominal->dorder);
    L.tr.order = nominal->dorder;
  }
  if (may_pair) L.tr.pair = use_pairs(nominal, L.f->vehicles);
  if (L.cls && L.slots) {  // mpcqp_set_class_pairing: pairs within classes, over the dispatch order where there is one
    enqueue_class_slots(L.f->vehicles, L.K, L.cls, L.tr.order, L.slots, s);
    L.tr.pair = true;
  }
  loop(s, L);
  const int rc = launched(name);
  if (rc == MPCQP_OK)
    nominal->launched_as(kind, L.tr.pair ? 2 : 1, L.f->vehicles,
                         L.cls && L.slots ? class_slot_waves(L.f->vehicles, L.K) : -1);
  return rc;
}
}  // namespace mpcqp

extern "C" {

int mpcqp_fleet_loop(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, int steps, void* stream) {
  int rc = check_fleet(nominal, relaxed, f);
  if (rc) return rc;
  if (steps < 0) return fail(MPCQP_E_ARG, "steps must be >= 0");
  if (f->vehicles == 0 || steps == 0) return MPCQP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const mpcqp::fleet_loop_t loop = mpcqp::fused_loop(nominal, relaxed, &mpcqp::HorizonKernels::loop);
  if (!loop) return run_graph(nominal, relaxed, f, steps, s);  // mid / long horizons, reproducible or debug mode
  return mpcqp::enqueue_fused_loop(nominal, relaxed, loop, "k_fleet_loop", MPCQP_LAUNCH_LOOP, true,
                                   {nullptr, f, steps}, s);
}

int mpcqp_fleet_loop_mixed(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const int32_t* cls, int steps,
                           void* stream) {
  if (!cls) return fail(MPCQP_E_ARG, "null cls");
  int rc = check_fleet(nominal, relaxed, f);
  if (rc) return rc;
  if (steps < 0) return fail(MPCQP_E_ARG, "steps must be >= 0");
  // the fused one-wave kernel only; refused before anything is enqueued or invalidated
  const mpcqp::fleet_loop_t loop = mpcqp::fused_loop(nominal, relaxed, &mpcqp::HorizonKernels::loop_mixed);
  if (!loop)
    return fail(MPCQP_E_HORIZON, "mpcqp_fleet_loop_mixed runs the fused one-wave loop only (N <= 32, fast mode, no "
                                 "debug_state): the stepped fleet has no per-vehicle classes");
  if ((rc = mpcqp::check_loop_classes(nominal, relaxed, "mpcqp_fleet_loop_mixed")) != MPCQP_OK) return rc;
  if (f->vehicles == 0 || steps == 0) return MPCQP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = mpcqp::grow_loop_classes(nominal, s)) != MPCQP_OK) return rc;
  mpcqp::LoopLaunch L{nullptr, f, steps};
  L.cls = cls;
  L.K = nominal->n_classes;
  if (mpcqp::use_class_pairs(nominal)) L.slots = nominal->dslots;  // two vehicles of one class per wave
  return mpcqp::enqueue_fused_loop(nominal, relaxed, loop, "k_fleet_loop_mixed", MPCQP_LAUNCH_LOOP_MIXED, false, L, s);
}

// mpcqp_fleet_loop_warm (carry == nullptr) and mpcqp_fleet_loop_warm_carry after their own argument
// checks; `who` names the caller in the refusal.  One vehicle per wave without a carried guess is
// k_fleet_loop_warm; a carried guess, or two vehicles per wave (MPCQP_PAIR_ON, N <= 15), is
// k_fleet_loop_warm_carry.
static int fleet_loop_warm(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, int steps, int guess_passes,
                           double* carry, const char* who, void* stream) {
  int rc = check_fleet(nominal, relaxed, f);
  if (rc) return rc;
  if (steps < 0) return fail(MPCQP_E_ARG, "steps must be >= 0");
  // the fused one-wave kernel only; refused before anything is enqueued or invalidated
  const mpcqp::fleet_loop_t loop = mpcqp::fused_loop(nominal, relaxed, &mpcqp::HorizonKernels::loop_warm);
  const mpcqp::fleet_loop_t loop_carry = mpcqp::fused_loop(nominal, relaxed, &mpcqp::HorizonKernels::loop_warm_carry);
  if (!loop || !loop_carry)
    return fail(MPCQP_E_HORIZON, std::string(who) + " runs the fused one-wave loop only (N <= 32, fast mode, no "
                                                    "debug_state): the stepped fleet takes no guess");
  if (f->vehicles == 0 || steps == 0) return MPCQP_OK;
  mpcqp::LoopLaunch L{nullptr, f, steps};
  L.guess_passes = guess_passes;
  L.carry = carry;
  L.tr.pair = mpcqp::use_pairs_warm(nominal);
  const bool carry_kernel = carry || L.tr.pair;
  return mpcqp::enqueue_fused_loop(nominal, relaxed, carry_kernel ? loop_carry : loop,
                                   carry_kernel ? "k_fleet_loop_warm_carry" : "k_fleet_loop_warm",
                                   carry ? MPCQP_LAUNCH_LOOP_WARM_CARRY : MPCQP_LAUNCH_LOOP_WARM, false, L,
                                   static_cast<hipStream_t>(stream));
}

int mpcqp_fleet_loop_warm(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, int steps, int guess_passes,
                          void* stream) {
  return fleet_loop_warm(nominal, relaxed, f, steps, guess_passes, nullptr, "mpcqp_fleet_loop_warm", stream);
}

int mpcqp_fleet_loop_warm_carry(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, int steps, int guess_passes,
                                double* U_carry, void* stream) {
  if (!U_carry) return fail(MPCQP_E_ARG, "null U_carry");
  return fleet_loop_warm(nominal, relaxed, f, steps, guess_passes, U_carry, "mpcqp_fleet_loop_warm_carry", stream);
}

int mpcqp_fleet_run(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, int steps, int use_graph,
                    void* stream) {
  int rc = check_fleet(nominal, relaxed, f);
  if (rc) return rc;
  if (steps < 0) return fail(MPCQP_E_ARG, "steps must be >= 0");
  if (f->vehicles == 0 || steps == 0) return MPCQP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (use_graph) return run_graph(nominal, relaxed, f, steps, s);
  for (int i = 0; i < steps; ++i) {
    rc = enqueue_step(nominal, relaxed, f, s);
    if (rc) return rc;
  }
  return MPCQP_OK;
}

}  // extern "C"
