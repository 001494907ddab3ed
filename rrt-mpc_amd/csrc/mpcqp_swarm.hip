// mpcqp_swarm.hip -- BASELINE config 5 on the device: the fleet closed loop with a per-step
// replan trigger and the replanning itself, no host round trip.
//
// One mpcqp_swarm_step = one closed-loop step of every vehicle, then replanning of the vehicles
// the step left off their reference:
//   fleet step          mpcqp_fleet.hip: window + nominal/relaxed MPC + plant + path_idx + goal
//                       (src/pipeline/control_stage.py:100-150)
//   k_swarm_trigger     the roadmap trigger of README.md:146-148: a RUNNING vehicle farther than
//                       replan_distance from ref[path_idx], or one the step ABORTED (QP unsolved
//                       after relaxation), with replans left -> MPCQP_FLEET_REPLAN_*, the RRT*
//                       problem {current position -> goal} and the PCG64 state of its next seed
//   k_swarm_plan        RRT* tree growth (rrt_star.py:201-248), flagged vehicles only
//   k_swarm_paths       path extraction + shortcut pruning (rrt_star.py:245-262, 376-389)
//   k_swarm_smooth      centripetal Catmull-Rom (rrt_star.py:104-159, 264-283)
//   k_swarm_refbuild    build_reference (ref_builder.py:10-22) into a staging buffer
//   k_swarm_commit      success -> the new reference, path_idx 0, RUNNING (pose, speed and u_prev
//                       carry over); failure -> the vehicle keeps its reference (RUNNING) or stays
//                       ABORTED; either way one replan is used
// Every replanning kernel exits at once for an unflagged vehicle, so a step without replans
// costs a handful of empty launches; mpcqp_swarm_run replays the whole step as a hipGraph.
// mpcqp_swarm_loop runs the same thing as max_replans + 1 launches of the fused fleet loop
// (k_fleet_loop with the trigger: each vehicle steps until it triggers or ends) with the replanning
// kernels in between -- no per-step launches.  mpcqp_swarm_loop_warm is the same rounds with
// k_swarm_loop_warm: each vehicle's solves start from its step before, cold at the first step of a launch.
// mpcqp_swarm_loop_mixed / _mixed_warm are the same rounds again with a parameter class per vehicle
// (k_swarm_loop_mixed, k_swarm_loop_mixed_warm); the replanning kernels read no parameter block.
// mpcqp_swarm_run_map / mpcqp_swarm_loop_map are the stepped and the fused swarm on a map that changes with a
// vehicle's step count: the trigger also fires for a reference that runs into a newly occupied cell
// (k_swarm_trigger_map; inside the fused loop k_swarm_loop_map), and k_swarm_plan_map / k_swarm_paths_map plan on
// the grid of the moment instead of s.occupancy.
#include "mpcqp_build.h"
#include "mpcqp_plan.h"
#include "mpcqp_refbuild.h"

namespace {
using mpcqp::fail;

constexpr int kCatmullCap = 4096;  // deduplicated points per path (LDS of k_swarm_smooth / k_catmull_rom)
constexpr int kRefCap = 6144;      // smoothed points per path that build_reference stages in LDS

__device__ __forceinline__ bool replanning(int ph) {
  return ph == MPCQP_FLEET_REPLAN_RUNNING || ph == MPCQP_FLEET_REPLAN_ABORTED;
}

__global__ __launch_bounds__(kWave) void k_swarm_trigger(mpcqp_fleet f, mpcqp_swarm s) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * kWave + threadIdx.x;
  if (v >= f.vehicles) return;
  const int ph = f.phase[v];
  const int used = s.replans[v];
  if (used < 0 || used >= s.max_replans) return;
  bool go = ph == MPCQP_FLEET_ABORTED;
  if (ph == MPCQP_FLEET_RUNNING && s.replan_distance > 0.0) {
    const int len = f.ref_len[v], pi = f.path_idx[v];
    if (len >= 1 && len <= f.ref_stride && pi >= 0 && pi < len) {
      go = swarm_off_track(f.state[(size_t)v * 4], f.state[(size_t)v * 4 + 1],
                           f.ref_global + ((size_t)v * f.ref_stride + pi) * 4, s.replan_distance);
    }
  }
  if (!go) return;
  f.phase[v] = ph == MPCQP_FLEET_ABORTED ? MPCQP_FLEET_REPLAN_ABORTED : MPCQP_FLEET_REPLAN_RUNNING;
  double* sg = s.start_goal + 4 * (size_t)v;
  sg[0] = f.state[(size_t)v * 4];
  sg[1] = f.state[(size_t)v * 4 + 1];
  sg[2] = f.goal[(size_t)v * 2];
  sg[3] = f.goal[(size_t)v * 2 + 1];
}

__global__ __launch_bounds__(kPlanThreads) void k_swarm_plan(mpcqp_fleet f, mpcqp_swarm s) {
  extern __shared__ double lds[];
  __shared__ PlanSmem sm;
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const int M = s.rrt.max_iterations + 2;
  const uint64_t* rs = s.rng_table + ((size_t)v * s.max_replans + s.replans[v]) * 4;
  rrt_grow_one(s.rrt, s.occupancy, s.start_goal + 4 * (size_t)v, nullptr, rs, s.nodes + (size_t)v * M * 4,
               s.count + v, s.meta + 2 * (size_t)v, lds, sm);
}

__global__ __launch_bounds__(kPlanThreads) void k_swarm_paths(mpcqp_fleet f, mpcqp_swarm s) {
  extern __shared__ double lds[];
  __shared__ PlanSmem sm;
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const size_t M = (size_t)s.rrt.max_iterations + 2;
  rrt_extract_one(s.rrt, s.prune, s.occupancy, s.nodes + (size_t)v * M * 4, s.count + v, s.meta + 2 * (size_t)v,
                  s.raw + (size_t)v * M * 2, s.raw_len + v, s.pruned + (size_t)v * M * 2, s.pruned_len + v, lds, sm);
}

// ---- the stepped swarm on a changing map (mpcqp_swarm_run_map): k_swarm_trigger with the blocked test
// after the off-track test (one thread per vehicle, the rows one after the other: the integer outcome of
// k_swarm_loop_map's whole-wave vote), grid_of and the cause; k_swarm_plan / k_swarm_paths on the vehicle's grid.
// Twins of the three kernels above on purpose: a shared __device__ body changed the instructions of the kernels
// on both sides, whichever way it took the map ("Fixed kernels").
__global__ __launch_bounds__(kWave) void k_swarm_trigger_map(mpcqp_fleet f, mpcqp_swarm s, mpcqp::LoopMap m) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * kWave + threadIdx.x;
  if (v >= f.vehicles) return;
  const int ph = f.phase[v];
  const int used = s.replans[v];
  if (used < 0 || used >= s.max_replans) return;
  int cause = ph == MPCQP_FLEET_ABORTED ? MPCQP_REPLAN_ABORTED : 0;
  if (ph == MPCQP_FLEET_RUNNING) {
    const int len = f.ref_len[v], pi = f.path_idx[v];
    if (len >= 1 && len <= f.ref_stride && pi >= 0 && pi < len) {
      const double* rows = f.ref_global + (size_t)v * f.ref_stride * 4;
      if (s.replan_distance > 0.0 &&
          swarm_off_track(f.state[(size_t)v * 4], f.state[(size_t)v * 4 + 1], rows + (size_t)pi * 4, s.replan_distance)) {
        cause = MPCQP_REPLAN_OFF_TRACK;
      } else {
        const uint8_t* grid = swarm_map_grid(m, f.steps[v]);
        for (int j = 0; j < m.lookahead && !cause; ++j)
          if (swarm_map_occupied(m, grid, rows + (size_t)min(pi + j, len - 1) * 4)) cause = MPCQP_REPLAN_BLOCKED;
      }
    }
  }
  if (!cause) return;
  f.phase[v] = ph == MPCQP_FLEET_ABORTED ? MPCQP_FLEET_REPLAN_ABORTED : MPCQP_FLEET_REPLAN_RUNNING;
  double* sg = s.start_goal + 4 * (size_t)v;
  sg[0] = f.state[(size_t)v * 4];
  sg[1] = f.state[(size_t)v * 4 + 1];
  sg[2] = f.goal[(size_t)v * 2];
  sg[3] = f.goal[(size_t)v * 2 + 1];
  swarm_map_note(m, mpcqp::LoopTrigger{s.replan_distance, s.max_replans, s.replans, s.start_goal}, v, f.steps[v], cause);
}

// the grid a flagged vehicle plans on: that of its trigger (grid_of, written by this launch sequence's trigger)
__device__ __forceinline__ const uint8_t* replan_grid(const mpcqp::LoopMap& m, int v) {
  const int g = max(0, min(m.grid_of[v], m.num_grids - 1));
  return m.grids + (size_t)g * m.height * m.width;
}

__global__ __launch_bounds__(kPlanThreads) void k_swarm_plan_map(mpcqp_fleet f, mpcqp_swarm s, mpcqp::LoopMap m) {
  extern __shared__ double lds[];
  __shared__ PlanSmem sm;
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const int M = s.rrt.max_iterations + 2;
  const uint64_t* rs = s.rng_table + ((size_t)v * s.max_replans + s.replans[v]) * 4;
  rrt_grow_one(s.rrt, replan_grid(m, v), s.start_goal + 4 * (size_t)v, nullptr, rs,
               s.nodes + (size_t)v * M * 4, s.count + v, s.meta + 2 * (size_t)v, lds, sm);
}

__global__ __launch_bounds__(kPlanThreads) void k_swarm_paths_map(mpcqp_fleet f, mpcqp_swarm s, mpcqp::LoopMap m) {
  extern __shared__ double lds[];
  __shared__ PlanSmem sm;
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const size_t M = (size_t)s.rrt.max_iterations + 2;
  rrt_extract_one(s.rrt, s.prune, replan_grid(m, v), s.nodes + (size_t)v * M * 4, s.count + v,
                  s.meta + 2 * (size_t)v, s.raw + (size_t)v * M * 2, s.raw_len + v, s.pruned + (size_t)v * M * 2,
                  s.pruned_len + v, lds, sm);
}

// the planner's final path (rrt_star.py:264-283): smoothed when spline_samples > 1 and the
// smoothing gives >= 2 points, else the pruned path; smooth_len -1 = over capacity
__device__ void final_path(const double* pruned, int plen, const mpcqp_swarm& s, double* out, int32_t* out_len,
                           double* lds) {
  const int lane = threadIdx.x;
  int k = -2;
  if (plen >= 2 && s.spline_samples > 1)
    k = catmull_rom_one(pruned, plen, s.spline_samples, s.spline_alpha, s.dedupe_tol, lds, kCatmullCap, out,
                        s.path_cap);
  if (k == -1) {
    if (lane == 0) *out_len = -1;
    return;
  }
  if (k < 2) {  // no (usable) smoothing: the pruned path itself
    if (plen > s.path_cap) {
      if (lane == 0) *out_len = -1;
      return;
    }
    for (int i = lane; i < 2 * plen; i += kWave) out[i] = pruned[i];
    k = plen;
  }
  if (lane == 0) *out_len = k;
}

__global__ __launch_bounds__(kWave) void k_swarm_smooth(mpcqp_fleet f, mpcqp_swarm s) {
  extern __shared__ double lds[];
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const size_t M = (size_t)s.rrt.max_iterations + 2;
  final_path(s.pruned + (size_t)v * M * 2, s.pruned_len[v], s, s.smooth + (size_t)v * s.path_cap * 2,
             s.smooth_len + v, lds);
}

__global__ __launch_bounds__(kWave) void k_swarm_refbuild(mpcqp_fleet f, mpcqp_swarm s) {
  extern __shared__ double lds[];
  const int v = blockIdx.x;
  if (v >= f.vehicles || !replanning(f.phase[v])) return;
  const int P = s.smooth_len[v];
  if (P < 1) {  // no plan (or over capacity): nothing to build
    if (threadIdx.x == 0) s.new_len[v] = 0;
    return;
  }
  build_reference_one(s.smooth + (size_t)v * s.path_cap * 2, P, s.path_cap < kRefCap ? s.path_cap : kRefCap,
                      s.desired_speed, s.horizon, s.dt, f.ref_stride, s.new_ref + (size_t)v * f.ref_stride * 4,
                      s.new_len + v, lds);
}

__global__ __launch_bounds__(kWave) void k_swarm_commit(mpcqp_fleet f, mpcqp_swarm s) {
  const int v = blockIdx.x;
  if (v >= f.vehicles) return;
  const int ph = f.phase[v];
  if (!replanning(ph)) return;
  const int len = s.new_len[v];
  const bool ok = s.meta[2 * (size_t)v + 1] >= 0 && len >= 1 && len <= f.ref_stride;
  if (ok) {
    double* dst = const_cast<double*>(f.ref_global) + (size_t)v * f.ref_stride * 4;
    const double* src = s.new_ref + (size_t)v * f.ref_stride * 4;
    for (int i = threadIdx.x; i < 4 * len; i += kWave) dst[i] = src[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int used = s.replans[v];
    if (s.replan_step) s.replan_step[(size_t)v * s.max_replans + used] = ok ? f.steps[v] : -f.steps[v] - 1;
    s.replans[v] = used + 1;
    if (ok) {
      const_cast<int32_t*>(f.ref_len)[v] = len;
      f.path_idx[v] = 0;
      f.phase[v] = MPCQP_FLEET_RUNNING;
    } else {
      f.phase[v] = ph == MPCQP_FLEET_REPLAN_ABORTED ? MPCQP_FLEET_ABORTED : MPCQP_FLEET_RUNNING;
    }
  }
}

// batched smoothing of V paths (mpcqp_catmull_rom): path v = in[v * in_stride .. + in_len[v]) points
__global__ __launch_bounds__(kWave) void k_catmull_rom(int V, const double* __restrict__ in, const int32_t* __restrict__ in_len,
                                                       int in_stride, int samples, double alpha, double tol,
                                                       double* __restrict__ out, int32_t* __restrict__ out_len,
                                                       int out_stride) {
  extern __shared__ double lds[];
  const int v = blockIdx.x;
  if (v >= V) return;
  const int k = catmull_rom_one(in + (size_t)v * in_stride * 2, in_len[v], samples, alpha, tol, lds, kCatmullCap,
                                out + (size_t)v * out_stride * 2, out_stride);
  if (threadIdx.x == 0) out_len[v] = k;
}

// need_occupancy == false: the calls on a changing map, which plan on their own grids
int check_swarm(const mpcqp_fleet* f, const mpcqp_swarm* s, bool need_occupancy = true) {
  if (!s) return fail(MPCQP_E_ARG, "null swarm");
  if (s->max_replans < 0) return fail(MPCQP_E_ARG, "max_replans must be >= 0");
  if (s->rrt.max_iterations < 1 || s->rrt.max_iterations > kMaxPlanIterations)
    return fail(MPCQP_E_ARG, "max_iterations outside [1, " + std::to_string(kMaxPlanIterations) + "]");
  if (s->rrt.width < 2 || s->rrt.height < 2) return fail(MPCQP_E_ARG, "grid must be at least 2 x 2");
  if (s->path_cap < 2) return fail(MPCQP_E_ARG, "path_cap must be >= 2");
  if (s->horizon < 1 || s->horizon > MPCQP_MAX_HORIZON) return fail(MPCQP_E_HORIZON, "bad swarm horizon");
  if (!(s->dt > 0.0) || !(s->desired_speed > 0.0)) return fail(MPCQP_E_ARG, "dt and desired_speed must be > 0");
  if (s->max_replans > 0 &&
      ((need_occupancy && !s->occupancy) || !s->rng_table || !s->replans || !s->start_goal || !s->nodes || !s->count || !s->meta ||
       !s->raw || !s->raw_len || !s->pruned || !s->pruned_len || !s->smooth || !s->smooth_len || !s->new_ref ||
       !s->new_len))
    return fail(MPCQP_E_ARG, "null swarm buffer");
  (void)f;
  return MPCQP_OK;
}

// the map's own checks (after check_swarm: s is valid), and the device's view of it
int check_map(const mpcqp_swarm* s, const mpcqp_swarm_map* m) {
  if (!m) return fail(MPCQP_E_ARG, "null swarm map");
  if (m->num_grids < 1) return fail(MPCQP_E_ARG, "num_grids must be >= 1");
  if (m->epoch_steps < 1) return fail(MPCQP_E_ARG, "epoch_steps must be >= 1");
  if (m->lookahead < 0 || m->lookahead > MPCQP_SWARM_MAP_MAX_LOOKAHEAD)
    return fail(MPCQP_E_ARG, "lookahead outside [0, " + std::to_string(MPCQP_SWARM_MAP_MAX_LOOKAHEAD) + "]");
  if (!m->grids) return fail(MPCQP_E_ARG, "null grids");
  if (s->max_replans > 0 && !m->grid_of) return fail(MPCQP_E_ARG, "null grid_of");
  return MPCQP_OK;
}

mpcqp::LoopMap loop_map(const mpcqp_swarm* s, const mpcqp_swarm_map* m) {
  mpcqp::LoopMap d;
  d.grids = m->grids;
  d.num_grids = m->num_grids;
  d.epoch_steps = m->epoch_steps;
  d.lookahead = m->lookahead;
  d.width = s->rrt.width;
  d.height = s->rrt.height;
  d.grid_of = m->grid_of;
  d.cause = m->replan_cause;
  return d;
}

size_t plan_lds(const mpcqp_rrt_params& p) {
  return ((size_t)(p.max_iterations + 2) * (3 * sizeof(double) + sizeof(int)) + 7) / 8 * 8;
}

struct ReplanLds {
  size_t plan, paths, smooth, refbuild;
  explicit ReplanLds(const mpcqp_swarm* s)
      : plan(plan_lds(s->rrt)),
        paths((size_t)(s->rrt.max_iterations + 2) * 2 * sizeof(double)),
        smooth(sizeof(double) * 2 * kCatmullCap),
        refbuild(sizeof(double) * 3 * (size_t)(s->path_cap < kRefCap ? s->path_cap : kRefCap)) {}
};

// The three replanning kernels that read the map, chosen once: those of the fixed map (s->occupancy), or
// their _map twins for the calls on a changing map.  Launched through these handles with one argument
// list (f, s, map), of which the fixed map's kernels take the first two.
struct MapKernels {
  const void *trigger, *plan, *paths;
};
MapKernels map_kernels(const mpcqp_swarm_map* m) {
  using K = const void*;
  return m ? MapKernels{(K)&k_swarm_trigger_map, (K)&k_swarm_plan_map, (K)&k_swarm_paths_map}
           : MapKernels{(K)&k_swarm_trigger, (K)&k_swarm_plan, (K)&k_swarm_paths};
}

// dynamic-LDS limits of the replanning kernels (outside any stream capture)
int set_replan_attrs(const mpcqp_swarm* s, const mpcqp_swarm_map* m) {
  const ReplanLds l(s);
  const MapKernels k = map_kernels(m);
  auto big = [](const void* kernel, size_t bytes) {
    return bytes > 65536 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)
                         : hipSuccess;
  };
  hipError_t e = big(k.plan, l.plan);
  if (e == hipSuccess) e = big(k.paths, l.paths);
  if (e == hipSuccess) e = big(reinterpret_cast<const void*>(&k_swarm_smooth), l.smooth);
  if (e == hipSuccess) e = big(reinterpret_cast<const void*>(&k_swarm_refbuild), l.refbuild);
  if (e != hipSuccess) return fail(MPCQP_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
  return MPCQP_OK;
}

// trigger (unless the fused loop already flagged the vehicles) + the replanning kernels
// m != nullptr (the calls on a changing map): the map's trigger, and the plan / paths kernels on each vehicle's grid
int enqueue_replan(const mpcqp_fleet* f, const mpcqp_swarm* s, const mpcqp_swarm_map* m, hipStream_t st,
                   bool trigger = true) {
  const int V = f->vehicles;
  if (s->max_replans == 0 || V == 0) return MPCQP_OK;
  mpcqp_fleet fv = *f;
  mpcqp_swarm sv = *s;
  mpcqp::LoopMap mv = m ? loop_map(s, m) : mpcqp::LoopMap{};
  void* args[] = {&fv, &sv, &mv};  // a launch error shows in launched() below, as after <<<>>>
  const MapKernels k = map_kernels(m);
  const ReplanLds l(s);
  const size_t lc = l.smooth, lr = l.refbuild;
  if (trigger) (void)hipLaunchKernel(k.trigger, dim3((V + kWave - 1) / kWave), dim3(kWave), args, 0, st);
  (void)hipLaunchKernel(k.plan, dim3(V), dim3(kPlanThreads), args, l.plan, st);
  (void)hipLaunchKernel(k.paths, dim3(V), dim3(kPlanThreads), args, l.paths, st);
  hipLaunchKernelGGL(k_swarm_smooth, dim3(V), dim3(kWave), lc, st, fv, sv);
  hipLaunchKernelGGL(k_swarm_refbuild, dim3(V), dim3(kWave), lr, st, fv, sv);
  hipLaunchKernelGGL(k_swarm_commit, dim3(V), dim3(kWave), 0, st, fv, sv);
  return mpcqp::launched("swarm replan");
}

// One closed-loop step after the caller's checks: the fleet step, then the trigger and the replanning (m: on the
// changing map)
int swarm_step(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
               const mpcqp_swarm_map* m, void* stream) {
  int rc = mpcqp_fleet_step(nominal, relaxed, f, stream);
  if (rc) return rc;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
    rc = set_replan_attrs(s, m);
    if (rc) return rc;
  }
  return enqueue_replan(f, s, m, st);
}

// mpcqp_swarm_run (m == nullptr) and mpcqp_swarm_run_map: `steps` steps, one by one or as a replayed hipGraph.
// map: the call is the map's (check_map refuses a null m); it plans on its own grids (no s->occupancy) and runs
// the fleet's checks before the capture.
int swarm_run(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
              const mpcqp_swarm_map* m, bool map, int steps, int use_graph, void* stream) {
  int rc = check_swarm(f, s, !map);
  if (rc) return rc;
  if (map && (rc = check_map(s, m)) != MPCQP_OK) return rc;
  if (steps < 0) return fail(MPCQP_E_ARG, "steps must be >= 0");
  if (!f || f->vehicles == 0 || steps == 0) return mpcqp_fleet_run(nominal, relaxed, f, 0, 0, stream);
  hipStream_t user = static_cast<hipStream_t>(stream);
  if (!use_graph) {
    for (int i = 0; i < steps; ++i) {
      rc = swarm_step(nominal, relaxed, f, s, m, stream);
      if (rc) return rc;
    }
    return MPCQP_OK;
  }
  if (map && (rc = mpcqp_fleet_run(nominal, relaxed, f, 0, 0, stream)) != MPCQP_OK) return rc;  // the fleet's checks
  return mpcqp::replay_graph(
      map ? "swarm map" : "swarm", user, steps,
      [&] {
        const int attrs = set_replan_attrs(s, m);
        return attrs != MPCQP_OK ? attrs : mpcqp::fleet_buffers(nominal, relaxed, user);
      },
      [&](hipStream_t s2) { return swarm_step(nominal, relaxed, f, s, m, s2); });
}

}  // namespace

extern "C" {

int mpcqp_catmull_rom(int V, const double* in, const int32_t* in_len, int in_stride, int samples, double alpha,
                      double dedupe_tol, double* out, int32_t* out_len, int out_stride, void* stream) {
  if (V < 0) return fail(MPCQP_E_ARG, "V must be >= 0");
  if (V == 0) return MPCQP_OK;
  if (!in || !in_len || !out || !out_len) return fail(MPCQP_E_ARG, "null argument");
  if (in_stride < 1 || out_stride < 1) return fail(MPCQP_E_ARG, "strides must be >= 1");
  const size_t lds = sizeof(double) * 2 * kCatmullCap;
  hipError_t e = hipSuccess;
  if (lds > 65536)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_catmull_rom), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  if (e != hipSuccess) return fail(MPCQP_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
  hipLaunchKernelGGL(k_catmull_rom, dim3(V), dim3(kWave), lds, static_cast<hipStream_t>(stream), V, in, in_len,
                     in_stride, samples, alpha, dedupe_tol, out, out_len, out_stride);
  return mpcqp::launched("k_catmull_rom");
}

int mpcqp_swarm_step(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s, void* stream) {
  const int rc = check_swarm(f, s);
  return rc ? rc : swarm_step(nominal, relaxed, f, s, nullptr, stream);
}

int mpcqp_swarm_run(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s, int steps,
                    int use_graph, void* stream) {
  return swarm_run(nominal, relaxed, f, s, nullptr, false, steps, use_graph, stream);
}

int mpcqp_swarm_run_map(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                        const mpcqp_swarm_map* m, int steps, int use_graph, void* stream) {
  return swarm_run(nominal, relaxed, f, s, m, true, steps, use_graph, stream);
}

// The five fused swarm calls after their own argument checks: max_replans + 1 rounds of the fused loop with
// the trigger inside -- every vehicle runs until it triggers or ends, the flagged ones are replanned; a
// vehicle's r-th trigger comes in round r - 1, so the last round triggers none.
// Cold (mpcqp_swarm_loop, and mpcqp_swarm_loop_map), a parameter block without the fused loop runs the
// stepped swarm to the end; warm, it is refused before anything is enqueued or invalidated.
// mixed != nullptr (mpcqp_swarm_loop_mixed, mpcqp_swarm_loop_mixed_warm): the same rounds with a class per
// vehicle (cls), k_swarm_loop_mixed / k_swarm_loop_mixed_warm under the two workspaces' class tables;
// `mixed` names the caller in the refusals, and neither has a stepped fallback.
// map (mpcqp_swarm_loop_map): k_swarm_loop_map (the blocked test inside the loop) and the replanning on each
// flagged vehicle's grid; one vehicle per wave, cold, no classes.
static int swarm_loop(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                      const mpcqp_swarm_map* m, bool map, bool warm, int guess_passes, void* stream,
                      const char* mixed = nullptr, const int32_t* cls = nullptr) {
  using HK = mpcqp::HorizonKernels;
  struct Variant {
    mpcqp::fleet_loop_t HK::*member;
    const char* name;
    int kind;
  };
  const Variant var =
      map ? Variant{&HK::swarm_map, "k_swarm_loop_map", MPCQP_LAUNCH_LOOP_MAP}
      : mixed ? (warm ? Variant{&HK::swarm_mixed_warm, "k_swarm_loop_mixed_warm", MPCQP_LAUNCH_LOOP_MIXED_WARM}
                      : Variant{&HK::swarm_mixed, "k_swarm_loop_mixed", MPCQP_LAUNCH_LOOP_MIXED})
              : (warm ? Variant{&HK::swarm_warm, "k_swarm_loop_warm", MPCQP_LAUNCH_LOOP_WARM}
                      : Variant{&HK::loop, "k_fleet_loop", MPCQP_LAUNCH_LOOP});
  int rc = check_swarm(f, s, !map);
  if (rc) return rc;
  if (map && (rc = check_map(s, m)) != MPCQP_OK) return rc;
  rc = mpcqp_fleet_loop(nominal, relaxed, f, 0, stream);  // the fleet's checks (no work at 0 steps)
  if (rc) return rc;
  const mpcqp::fleet_loop_t loop = mpcqp::fused_loop(nominal, relaxed, var.member);
  if (mixed && !loop)
    return fail(MPCQP_E_HORIZON, std::string(mixed) + " runs the fused one-wave loop only (N <= 32, fast mode, no "
                                                      "debug_state): the stepped swarm has no per-vehicle classes");
  if (warm && !loop)
    return fail(MPCQP_E_HORIZON, "mpcqp_swarm_loop_warm runs the fused one-wave loop only (N <= 32, fast mode, no "
                                 "debug_state): the stepped swarm takes no guess");
  if (mixed) {
    if ((rc = mpcqp::check_loop_classes(nominal, relaxed, mixed)) != MPCQP_OK) return rc;
    // one dt: the replanning builds every vehicle's new reference with s->dt
    for (const mpcqp_ws* ws : {nominal, relaxed})
      for (size_t k = 0; k < ws->hclasses.size(); ++k)
        if (ws->hclasses[k].dt != s->dt)
          return fail(MPCQP_E_ARG, std::string(mixed) + ": class " + std::to_string(k) + " of the " +
                                       (ws == nominal ? "nominal" : "relaxed") + " table has dt " +
                                       std::to_string(ws->hclasses[k].dt) + ", the swarm " + std::to_string(s->dt) +
                                       " (one dt: the replanning builds references with the swarm's)");
  }
  if (f->vehicles == 0) return MPCQP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (s->max_replans > 0 && (rc = set_replan_attrs(s, m)) != MPCQP_OK) return rc;
  if (!loop)  // mid / long horizons, reproducible or debug mode: the stepped swarm to the end
    return swarm_run(nominal, relaxed, f, s, m, map, f->max_steps, 1, stream);
  if (mixed && (rc = mpcqp::grow_loop_classes(nominal, st)) != MPCQP_OK) return rc;
  mpcqp::LoopLaunch L{nullptr, f, f->max_steps, {s->replan_distance, s->max_replans, s->replans, s->start_goal}};
  if (warm) L.guess_passes = guess_passes;
  if (map) L.map = loop_map(s, m);
  if (mixed) {
    L.cls = cls;
    L.K = nominal->n_classes;
  } else if (warm) {
    L.tr.pair = mpcqp::use_pairs_warm(nominal);
  }
  for (int r = 0; r <= s->max_replans; ++r) {
    rc = mpcqp::enqueue_fused_loop(nominal, relaxed, loop, var.name, var.kind, !warm && !mixed && !map, L, st);
    if (rc) return rc;
    if (r < s->max_replans && (rc = enqueue_replan(f, s, m, st, false)) != MPCQP_OK) return rc;
  }
  return MPCQP_OK;
}

int mpcqp_swarm_loop(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s, void* stream) {
  return swarm_loop(nominal, relaxed, f, s, nullptr, false, false, 0, stream);
}

int mpcqp_swarm_loop_warm(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                          int guess_passes, void* stream) {
  return swarm_loop(nominal, relaxed, f, s, nullptr, false, true, guess_passes, stream);
}

int mpcqp_swarm_loop_mixed(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                           const int32_t* cls, void* stream) {
  if (!cls) return fail(MPCQP_E_ARG, "null cls");
  return swarm_loop(nominal, relaxed, f, s, nullptr, false, false, 0, stream, "mpcqp_swarm_loop_mixed", cls);
}

int mpcqp_swarm_loop_mixed_warm(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                                const int32_t* cls, int guess_passes, void* stream) {
  if (!cls) return fail(MPCQP_E_ARG, "null cls");
  return swarm_loop(nominal, relaxed, f, s, nullptr, false, true, guess_passes, stream, "mpcqp_swarm_loop_mixed_warm",
                    cls);
}

int mpcqp_swarm_loop_map(mpcqp_ws* nominal, mpcqp_ws* relaxed, const mpcqp_fleet* f, const mpcqp_swarm* s,
                         const mpcqp_swarm_map* m, void* stream) {
  return swarm_loop(nominal, relaxed, f, s, m, true, false, 0, stream);
}

}  // extern "C"
