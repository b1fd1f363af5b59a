// tfg_engine.hip -- MI355X (gfx950) glacier energy-balance engine: kernels and
// the C ABI declared in include/tfg.h.  The fused step kernel k_fused is in
// tfg_fused.hpp; its fp64 instantiations are compiled in tfg_fused_f64.hip.
//
// Hot path: k_fused<R, EXACT, READ_DEPTHS, CATCH> advances every cell of the
// shard by K consecutive time steps in ONE launch.  A thread owns C adjacent
// cells (C*sizeof(R) = 16 B: one dwordx4 per field per wave-lane); it loads the
// cells' static rasters and fp64 state once, keeps the state in registers for
// the K steps, and per step streams in the step's forcing frame and the
// expiring snowfall-window slot and streams out the new slot and the six BMI
// outputs.  There is no lateral coupling in the reference physics (Qc = Qa = 0,
// bmi_topoflow_glacier.py:936-955), so no LDS tile or halo is needed; LDS only
// holds the per-wave mass-balance bins.
//
// Mass-balance diagnostics (vol_P/PR/PS/SM/IM, P_max: :558-624, :1482-1494)
// are reduced without atomics: lane registers -> wave butterfly (__shfl_xor) ->
// per-wave LDS bins -> one slab row per workgroup (accumulated over launches)
// -> k_diag_reduce when the diagnostics are read, which folds
// the slab into the running fp64 totals in a fixed order (bitwise
// reproducible).
//
// Layout: the one-cell kernels and the small grid kernels (with tfg_flow.hpp,
// tfg_series.hpp, tfg_forcing.hpp); then the host layer.  What a handle owns
// is a member that releases itself (Buf of tfg_hostbuf.hpp over three memory
// policies, Event, Stream, StageRing, MappedBlock), so tfg_destroy is `delete`.
// One definition each: by_type / by_types (the float | double instance of a
// launch), read_flag and note_written (finite-data tracking), wait_flags,
// step_args, kBmiToPlane; for the history readers hist_window (the checked slots,
// in batches) and one scratch (reserve_idle).  Then the C ABI, in include/tfg.h's order.
#include <hip/hip_runtime.h>
#include <mutex>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tfg.h"
#include "tfg_physics.hpp"
#include "tfg_conduction.hpp"
#include "tfg_fused.hpp"
#include "tfg_hostbuf.hpp"

namespace {

using namespace tfg_kern;

// One step of a one-cell fp64 handle for tfg_update (the single-catchment BMI
// update(), :413-465, one model per catchment as NextGen runs it): the step's
// inputs and uniforms arrive as kernel arguments, one workgroup of four waves
// (one per SIMD) runs the step with its transcendental calls batched across
// lanes and function classes across waves (cell_step_exact_wave), and
// thread 0 writes the state, the window slot, the history slot, the frame, the
// eight outputs into the pinned host block, the diagnostic slab row and the
// release flag.  Same arithmetic as k_fused<double, true, ...> with K = 1, so
// the same outputs and state bit for bit (the diagnostics to fp64 rounding,
// see k_cell_run); the per-launch fixed work (LDS bins, the
// read-back of the history slot, host-memory reads of inputs and uniforms) is
// gone from the critical path.
struct CellIo {
  tfg_uniforms u;
  double in[kNumForc];  // P, T_air, Hum_sp, P_air, uz (device frame order)
};

// The one cell's fp64 state (the depths read or re-derived as k_fused does)
// and its static geometry (k_prepare_static's planes).
__device__ __forceinline__ void load_one_cell(const DevParams& p, int64_t np, const double* __restrict__ st,
                                              const int64_t* __restrict__ tot, const double* __restrict__ geo,
                                              int read_depths, CellState& cs, CellStatic& sx) {
  cs.h_swe = st[S_HSWE * np];
  cs.h_iwe = st[S_HIWE * np];
  cs.Eccs = st[S_ECCS * np];
  cs.Ecci = st[S_ECCI * np];
  cs.n = st[S_N * np];
  cs.albedo = st[S_ALB * np];
  if (read_depths) {
    cs.h_snow = st[S_HSNOW * np];
    cs.h_ice = st[S_HICE * np];
  } else {
    cs.h_snow = cs.h_swe * p.ws;  // :1711, bit-identical to the last step
    cs.h_ice = cs.h_iwe * p.wi;   // :1726
  }
  cs.tot_q = tot[0];
  sx = {geo[0], geo[np], geo[2 * np], geo[3 * np], geo[4 * np], geo[5 * np], geo[6 * np]};
}

// Write the state back and add the step(s)' diagnostics to the slab row `srow`
// (whose values at kernel start were `sv`) as k_fused accumulates them: the
// wave and workgroup sums of one cell add zeros.
__device__ __forceinline__ void store_one_cell(int64_t np, const CellState& cs, const CellDiag& d, const double (&sv)[6],
                                               double* __restrict__ st, int64_t* __restrict__ tot,
                                               double* __restrict__ srow) {
  st[S_HSWE * np] = cs.h_swe;
  st[S_HIWE * np] = cs.h_iwe;
  st[S_ECCS * np] = cs.Eccs;
  st[S_ECCI * np] = cs.Ecci;
  st[S_N * np] = cs.n;
  st[S_ALB * np] = cs.albedo;
  tot[0] = cs.tot_q;
  srow[0] = sv[0] + d.P;
  srow[1] = sv[1] + d.PR;
  srow[2] = sv[2] + d.PS;
  srow[3] = sv[3] + d.SM;
  srow[4] = sv[4] + d.IM;
  srow[5] = tfg::npmax(sv[5], d.Pmax);
}

// The step's six history planes into history slot `slot`.
__device__ __forceinline__ void store_one_hist(int64_t np, int slot, const CellOut& o, double* __restrict__ hist) {
  double* h = hist + (int64_t)slot * kNumHist * np;
  h[H_HSNOW * np] = o.h_snow;
  h[H_SM * np] = o.SM;
  h[H_HICE * np] = o.h_ice;
  h[H_IM * np] = o.IM;
  h[H_MTOT * np] = o.M_total;
  h[H_RH * np] = o.RH;
}

// The step's eight BMI outputs: h_snow, h_swe, SM, h_ice, h_iwe, IM, M_total, RH.
__device__ __forceinline__ void store_one_out(const CellState& cs, const CellOut& o, double* __restrict__ out) {
  out[0] = o.h_snow;
  out[1] = cs.h_swe;
  out[2] = o.SM;
  out[3] = o.h_ice;
  out[4] = cs.h_iwe;
  out[5] = o.IM;
  out[6] = o.M_total;
  out[7] = o.RH;
}

__global__ __launch_bounds__(64 * tfg::kCellWaves) void k_cell(const KArgs a, const CellIo io, const double* __restrict__ geo,
                                             const int32_t* __restrict__ catch_id, double* __restrict__ st,
                                             int64_t* __restrict__ tot, int32_t* __restrict__ ring,
                                             double* __restrict__ forc, double* __restrict__ hist,
                                             double* __restrict__ slab, const double* __restrict__ qcf,
                                             int read_depths) {
  __shared__ double lds_x[tfg::X_SLOTS * 4];
  const DevParams& p = a.p;
  const int64_t np = a.n_pad;
  const tfg_uniforms& u = io.u;
#ifdef TFG_CELL_TIMING  // diagnostic build: phase times [wall-clock ticks] replace the outputs
  const long long tt0 = wall_clock64();
#endif
  CellState cs;
  CellStatic sx;
  load_one_cell(p, np, st, tot, geo, read_depths, cs, sx);
  const int32_t q_old = ring[(int64_t)u.slot * np];
  double* srow = slab + (catch_id ? catch_id[0] : 0) * 6;
  double sv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) sv[i] = srow[i];
  const double qc = qcf ? qcf[0] : 0.0;
  CellDiag d;
  diag_zero(d);
  CellOut o;
  int32_t q_new;
#ifdef TFG_CELL_TIMING
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  asm volatile("" ::"v"(cs.h_swe), "v"(sx.elev), "v"(sv[0]), "v"(q_old));
  const long long tt1 = wall_clock64();
#endif
  tfg::cell_step_exact_wave<tfg::kCellWaves>(p, sx, u, io.in[F_P], io.in[F_T], io.in[F_Q], io.in[F_PA], io.in[F_UZ],
                                              q_old, q_new, cs, o, d, qc, lds_x);
#ifdef TFG_CELL_TIMING
  asm volatile("" ::"v"(o.SM), "v"(o.RH), "v"(cs.Eccs), "v"(o.h_snow), "v"(d.SM));
  const long long tt2 = wall_clock64();
#endif
  if (threadIdx.x == 0) {
    ring[(int64_t)u.slot * np] = q_new;
    store_one_hist(np, u.hist, o, hist);
    double* fr = forc + (int64_t)u.frame * kNumForc * np;
#pragma unroll
    for (int f = 0; f < kNumForc; ++f) fr[f * np] = io.in[f];
    store_one_cell(np, cs, d, sv, st, tot, srow);
    double* out = a.io_out;  // [8][1]
    store_one_out(cs, o, out);
#ifdef TFG_CELL_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long tt3 = wall_clock64();
    out[0] = (double)(tt1 - tt0);
    out[1] = (double)(tt2 - tt1);
    out[2] = (double)(tt3 - tt2);
#endif
    __threadfence_system();
    __hip_atomic_store(a.io_flag, a.io_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// K consecutive steps of a one-cell fp64 handle (tfg_step: update_until and
// bulk runs of one catchment): k_cell's lane-batched step in a loop, the state
// in registers, each step's frame values, window slot and uniforms requested
// one step ahead (a one-slot window runs one step per launch, tfg_step).
// Same arithmetic as k_fused<double, true, ...>, so the same outputs and state
// bit for bit.  The diagnostics agree to fp64 rounding only (1e-12 relative,
// tests/test_gpu_diagnostics.py): the one-cell kernels scale every step's terms
// by da dt (cell_step_exact_wave), k_fused sums them unscaled over a launch and
// scales once (diag_scale), so the fp64 grid's own diagnostics also move in
// their last bits with the launch partition.  Every thread stores the same
// values to the same addresses, so no
// store sits behind a branch and each wave reads back only window slots it
// wrote itself.
__global__ __launch_bounds__(64 * tfg::kCellWaves) void k_cell_run(const KArgs a, const tfg_uniforms* __restrict__ uni,
                                                 const double* __restrict__ geo, const int32_t* __restrict__ catch_id,
                                                 double* __restrict__ st, int64_t* __restrict__ tot,
                                                 int32_t* __restrict__ ring, const double* __restrict__ forc,
                                                 double* __restrict__ hist, double* __restrict__ slab,
                                                 const double* __restrict__ qcf, int read_depths) {
  __shared__ double lds_x[tfg::X_SLOTS * 4];
  const DevParams& p = a.p;
  const int64_t np = a.n_pad;
  CellState cs;
  CellStatic sx;
  load_one_cell(p, np, st, tot, geo, read_depths, cs, sx);
  double* srow = slab + (catch_id ? catch_id[0] : 0) * 6;
  double sv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) sv[i] = srow[i];
  const double qc = qcf ? qcf[0] : 0.0;
  CellDiag d;
  diag_zero(d);
  struct In {
    double v[kNumForc];
    int32_t q;
  };
  auto fetch = [&](int k, In& x) {
    const tfg_uniforms* un = uni + (k < a.K ? k : a.K - 1);
    const double* fr = forc + (int64_t)un->frame * kNumForc * np;
#pragma unroll
    for (int f = 0; f < kNumForc; ++f) x.v[f] = fr[f * np];
    x.q = ring[(int64_t)un->slot * np];
  };
  In cur, nxt;
  fetch(0, cur);
  for (int k = 0; k < a.K; ++k) {
    TFG_STEP_PARAMS(p);  // per-step constants (-2.5 % per step, same-box A/B, scripts/gpu_ab_cellrun.sh)
    fetch(k + 1, nxt);
    const tfg_uniforms u = uni[k];
    CellOut o;
    int32_t q_new;
    tfg::cell_step_exact_wave<tfg::kCellWaves>(p, sx, u, cur.v[F_P], cur.v[F_T], cur.v[F_Q], cur.v[F_PA], cur.v[F_UZ],
                                                cur.q, q_new, cs, o, d, qc, lds_x);
    ring[(int64_t)u.slot * np] = q_new;
    store_one_hist(np, u.hist, o, hist);
    cur = nxt;
  }
  store_one_cell(np, cs, d, sv, st, tot, srow);
}

// One step of many one-cell fp64 handles in one launch (tfg_update_many: the
// per-catchment BMI models of a process that have each been asked for a step;
// NextGen-style ensembles stepped together).  Workgroup j runs job j exactly
// as k_cell runs its one handle: the job record (the handle's DevParams and
// buffers, the step's uniforms and inputs) sits in a pinned, device-mapped
// host block; the workgroup stages it into LDS with one coalesced read, so
// every later uniform read is an LDS broadcast instead of a PCIe round trip.
struct CellJob {
  DevParams p;
  tfg_uniforms u;
  double in[kNumForc];  // P, T_air, Hum_sp, P_air, uz (device frame order)
  const double* geo;
  const int32_t* catch_id;
  double* st;
  int64_t* tot;
  int32_t* ring;
  double* forc;
  double* hist;
  double* slab;
  const double* qc;  // null while the conduction term is off
  int64_t n_pad;
  int32_t read_depths;
  int32_t pad_;
};
static_assert(sizeof(CellJob) % 8 == 0, "CellJob is staged as 8-byte words");

__global__ __launch_bounds__(64 * tfg::kCellWaves) void k_cell_many(const CellJob* __restrict__ jobs,
                                                  double* __restrict__ out, uint32_t* __restrict__ flags,
                                                  uint32_t seq) {
  __shared__ double lds_x[tfg::X_SLOTS * 4];
  __shared__ CellJob job;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(jobs + blockIdx.x);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&job);
    for (int i = threadIdx.x; i < (int)(sizeof(CellJob) / 8); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const DevParams& p = job.p;
  const int64_t np = job.n_pad;
  double* const st = job.st;
  int64_t* const tot = job.tot;
  int32_t* const ring = job.ring;
  CellState cs;
  CellStatic sx;
  load_one_cell(p, np, st, tot, job.geo, job.read_depths, cs, sx);
  const int32_t q_old = ring[(int64_t)job.u.slot * np];
  double* srow = job.slab + (job.catch_id ? job.catch_id[0] : 0) * 6;
  double sv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) sv[i] = srow[i];
  const double qc = job.qc ? job.qc[0] : 0.0;
  CellDiag d;
  diag_zero(d);
  CellOut o;
  int32_t q_new;
  tfg::cell_step_exact_wave<tfg::kCellWaves>(p, sx, job.u, job.in[F_P], job.in[F_T], job.in[F_Q], job.in[F_PA],
                                              job.in[F_UZ], q_old, q_new, cs, o, d, qc, lds_x);
  if (threadIdx.x == 0) {
    ring[(int64_t)job.u.slot * np] = q_new;
    store_one_hist(np, job.u.hist, o, job.hist);
    double* fr = job.forc + (int64_t)job.u.frame * kNumForc * np;
#pragma unroll
    for (int f = 0; f < kNumForc; ++f) fr[f * np] = job.in[f];
    store_one_cell(np, cs, d, sv, st, tot, srow);
    store_one_out(cs, o, out + (int64_t)blockIdx.x * 8);
    __threadfence_system();
    __hip_atomic_store(flags + blockIdx.x, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Per-cell solar geometry of the fast engine, once per static-raster change:
// kGeoF fp32 planes then [tan(eq_lat), t_noon] fp64 (tfg::derive_geo).
template <class R>
__global__ void k_prepare_geo(const DevParams p, const R* __restrict__ stat, float* __restrict__ geo, int64_t n_pad) {
  double* gd = reinterpret_cast<double*>(geo + tfg::kGeoF * n_pad);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * blockDim.x) {
    const tfg::CellGeo g = tfg::derive_geo(p, (double)stat[i], (double)stat[n_pad + i], (double)stat[2 * n_pad + i]);
#pragma unroll
    for (int f = 0; f < tfg::kGeoF; ++f) geo[f * n_pad + i] = g.f[f];
    gd[i] = g.tan_eq;
    gd[n_pad + i] = g.t_noon;
  }
}

// Exact engine: CellStatic planes [kStaticPlanes][n_pad] fp64 (elev, cos_leq,
// sin_leq, dlon, tan_eq, cos_dlon, sin_dlon), derived once per static-raster
// change instead of once per launch.
template <class R>
__global__ void k_prepare_static(const DevParams p, const R* __restrict__ stat, double* __restrict__ gx, int64_t n_pad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * blockDim.x) {
    const CellStatic s = tfg::derive_static(p, (double)stat[i], (double)stat[n_pad + i], (double)stat[2 * n_pad + i]);
    gx[i] = s.elev;
    gx[n_pad + i] = s.cos_leq;
    gx[2 * n_pad + i] = s.sin_leq;
    gx[3 * n_pad + i] = s.dlon;
    gx[4 * n_pad + i] = s.tan_eq;
    gx[5 * n_pad + i] = s.cos_dlon;
    gx[6 * n_pad + i] = s.sin_dlon;
  }
}

// acc[i] = reduce over workgroups of slab[b][i]; one workgroup per diag entry.
__global__ __launch_bounds__(kBlock) void k_diag_reduce(const double* __restrict__ slab, int nblocks, int nb,
                                                        double* __restrict__ acc) {
  __shared__ double red[kBlock];
  const int i = blockIdx.x;
  const bool is_max = (i % 6) == 5;
  double v = is_max ? -INFINITY : 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) {
    const double x = slab[(int64_t)b * nb + i];
    v = is_max ? tfg::npmax(v, x) : v + x;
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const double o = red[threadIdx.x + s];
      red[threadIdx.x] = is_max ? tfg::npmax(red[threadIdx.x], o) : red[threadIdx.x] + o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) acc[i] = red[0];
}

template <class D, class S>
__global__ void k_convert(D* __restrict__ dst, const S* __restrict__ src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = (D)src[i];
}

// initialize() state (:389-395, :369, :288, :296) from the current depths
__global__ void k_init_state(double* __restrict__ st, int64_t n_pad, double rhoCp_snow, double del_T,
                             double Ecci0, int albedo_f32) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * blockDim.x) {
    const double e = rhoCp_snow * st[S_HSNOW * n_pad + i] * del_T;
    st[S_ECCS * n_pad + i] = tfg::npmax(e, 0.0);
    st[S_ECCI * n_pad + i] = Ecci0;
    st[S_N * n_pad + i] = 0.0;
    if (albedo_f32) reinterpret_cast<float*>(st + S_ALB * n_pad)[i] = 0.3f;  // the fp32 engine's albedo plane
    else st[S_ALB * n_pad + i] = 0.3;
  }
}

// materialise previous-step depths before a host overwrite of a depth field
__global__ void k_materialise_depths(double* __restrict__ st, int64_t n_pad, double ws, double wi) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * blockDim.x) {
    st[S_HSNOW * n_pad + i] = st[S_HSWE * n_pad + i] * ws;
    st[S_HICE * n_pad + i] = st[S_HIWE * n_pad + i] * wi;
  }
}

template <class R>
__global__ void k_check_slope(const R* __restrict__ slope, int64_t n, int32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (slope[i] < (R)0) atomicOr(flag, 1);
}

// --- synthetic workload (mirror: topoflow_glacier/synthetic.py) -----------
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float hash_u01(uint64_t seed, uint64_t field, uint64_t frame, uint64_t cell) {
  const uint64_t k = (field << 58) ^ (frame << 42) ^ cell;
  return (float)(splitmix64(seed ^ splitmix64(k)) >> 40) * 0x1p-24f;
}

template <class R>
__global__ void k_fill_synthetic(R* __restrict__ forc, R* __restrict__ stat, double* __restrict__ st,
                                 int64_t n, int64_t n_pad, int64_t nx, int64_t row0, int64_t nx_global,
                                 uint64_t seed, const float* __restrict__ diurnal, int n_frames) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nx, c = i % nx;
    const uint64_t cell = (uint64_t)((row0 + r) * nx_global + c);
    const float Tbar = -8.0f + 16.0f * hash_u01(seed, 6, 0, cell);
    stat[i] = (R)(1500.0f + 1500.0f * hash_u01(seed, 7, 0, cell));
    stat[n_pad + i] = (R)(0.5f + 99.5f * hash_u01(seed, 8, 0, cell));
    stat[2 * n_pad + i] = (R)(360.0f * hash_u01(seed, 9, 0, cell));
    const float h_swe = 0.25f * (0.8f + 0.4f * hash_u01(seed, 10, 0, cell));
    const float h_iwe = 1.834f * (0.8f + 0.4f * hash_u01(seed, 11, 0, cell));
    st[S_HSWE * n_pad + i] = (double)h_swe;
    st[S_HIWE * n_pad + i] = (double)h_iwe;
    st[S_HSNOW * n_pad + i] = (double)(h_swe * 20.0f);
    st[S_HICE * n_pad + i] = (double)(h_iwe * 1.0905125f);
    for (int f = 0; f < n_frames; ++f) {
      R* fr = forc + (int64_t)f * kNumForc * n_pad;
      const float T = (Tbar + 5.0f * diurnal[f]) + 2.0f * (hash_u01(seed, 0, f, cell) - 0.5f);
      const float q = 0.0019f + 0.0042f * hash_u01(seed, 1, f, cell);
      const float pa = 87100.0f + 2600.0f * hash_u01(seed, 2, f, cell);
      const float uz = 0.28f + 15.5f * hash_u01(seed, 3, f, cell);
      const float P = (hash_u01(seed, 4, f, cell) < 0.24f) ? 5.2e-7f * hash_u01(seed, 5, f, cell) : 0.0f;
      fr[F_P * n_pad + i] = (R)P;
      fr[F_T * n_pad + i] = (R)T;
      fr[F_Q * n_pad + i] = (R)q;
      fr[F_PA * n_pad + i] = (R)pa;
      fr[F_UZ * n_pad + i] = (R)uz;
    }
  }
}

thread_local std::string g_err;  // errors before a handle exists (per calling thread)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

}  // namespace

// ===========================================================================
// Handle
// ===========================================================================
// Horn's 3x3 slope/aspect (tfg_terrain_from_dem).  halo: [2][nx] fp64, the
// rows north of row 0 and south of row ny-1.  fp64, contraction off, so the
// numpy restatement in tests reproduces it up to libm rounding.
template <class R>
__global__ void k_terrain(const R* __restrict__ elev, const double* __restrict__ halo, R* __restrict__ slope,
                          R* __restrict__ aspect, int64_t ny, int64_t nx, double inv8dx, double inv8dy) {
#pragma clang fp contract(off)
  const int64_t n = ny * nx;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nx, c = i % nx;
    const int64_t cw = c > 0 ? c - 1 : c, ce = c < nx - 1 ? c + 1 : c;
    auto z = [&](int64_t rr, int64_t cc) -> double {
      if (rr < 0) return halo[cc];
      if (rr >= ny) return halo[nx + cc];
      return (double)elev[rr * nx + cc];
    };
    const double a = z(r - 1, cw), b = z(r - 1, c), cc_ = z(r - 1, ce);
    const double d = z(r, cw), f = z(r, ce);
    const double g = z(r + 1, cw), hh = z(r + 1, c), ii = z(r + 1, ce);
    const double dzdx = ((cc_ + 2.0 * f + ii) - (a + 2.0 * d + g)) * inv8dx;   // east
    const double dzds = ((g + 2.0 * hh + ii) - (a + 2.0 * b + cc_)) * inv8dy;  // south
    slope[i] = (R)sqrt(dzdx * dzdx + dzds * dzds);
    // downslope direction (-dz/dx, -dz/dnorth) = (-dzdx, +dzds), CCW from east
    aspect[i] = (R)((dzdx == 0.0 && dzds == 0.0) ? 0.0 : atan2(dzds, -dzdx));
  }
}


#include "tfg_flow.hpp"  // the optional ice-flow kernels (tfg_ice_flow_*)
#include "tfg_series.hpp"  // per-catchment sums of history planes (tfg_catchment_series)
#include "tfg_bands.hpp"  // per-catchment, per-elevation-band sums and counts of history planes (tfg_band_series)
#include "tfg_aggregate.hpp"  // per-cell time aggregates of history planes (tfg_cell_aggregate)
#include "tfg_forcing.hpp"  // forcing spread over the grid: per catchment (tfg_set_catchment_forcing), regridded (tfg_set_gridded_forcing)
#include "tfg_coarse.hpp"  // per-node sums and counts of history planes on a coarse grid (tfg_coarse_series)
#include "tfg_raster.hpp"  // polygons filled into the catchment-id raster (tfg_rasterize_polygons)

// tfg_set_inputs / tfg_get_outputs: the per-step BMI traffic of one call each.
// src [5][n]: P_air, Hum_sp, P, T_air, uz (BMI order) -> frame planes.
template <class R, class S>
__global__ void k_scatter_inputs(R* __restrict__ fr, const S* __restrict__ src, int64_t n, int64_t n_pad) {
  const int map[5] = {F_PA, F_Q, F_P, F_T, F_UZ};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
    for (int f = 0; f < 5; ++f) fr[map[f] * n_pad + i] = (R)src[f * n + i];
}
// dst [8][n]: h_snow, h_swe, SM, h_ice, h_iwe, IM, M_total, RH.  Before the
// first step (depths not yet derived) the depths come from the fp64 state.
template <class R, class D>
__global__ void k_gather_outputs(D* __restrict__ dst, const R* __restrict__ hs, const double* __restrict__ st, int64_t n,
                                 int64_t n_pad, int depths_from_state) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    dst[0 * n + i] = depths_from_state ? (D)st[S_HSNOW * n_pad + i] : (D)hs[H_HSNOW * n_pad + i];
    dst[1 * n + i] = (D)st[S_HSWE * n_pad + i];
    dst[2 * n + i] = (D)hs[H_SM * n_pad + i];
    dst[3 * n + i] = depths_from_state ? (D)st[S_HICE * n_pad + i] : (D)hs[H_HICE * n_pad + i];
    dst[4 * n + i] = (D)st[S_HIWE * n_pad + i];
    dst[5 * n + i] = (D)hs[H_IM * n_pad + i];
    dst[6 * n + i] = (D)hs[H_MTOT * n_pad + i];
    dst[7 * n + i] = (D)hs[H_RH * n_pad + i];
  }
}

// Snowfall-window checkpoint I/O (TFG_ST_WINDOW): metres <-> fixed point, and
// the running total rebuilt from the slots.
__global__ void k_window_set(int32_t* __restrict__ slot, const double* __restrict__ v, int64_t n, double qscale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    slot[i] = tfg::window_q(v[i], qscale);
}
__global__ void k_window_get(double* __restrict__ v, const int32_t* __restrict__ slot, int64_t n, double inv_qscale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = slot[i] == tfg::kWindowNan ? (double)NAN : (double)slot[i] * inv_qscale;
}
__global__ void k_window_total(int64_t* __restrict__ tot, const int32_t* __restrict__ ring, int ring_len, int64_t n_pad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = 0;
    for (int s = 0; s < ring_len; ++s) t += tfg::window_tot(ring[(int64_t)s * n_pad + i]);
    tot[i] = t;
  }
}

// Non-finite checks behind the fp32 engine's choice of step form (see
// tfg_handle::plane_state): flag |= 1 where a value is NaN or infinite, or
// where a window total holds a NaN slot.
// Planes of n cells at a stride of `stride` elements (padding cells excluded:
// they are computed along, from zero inputs, and may hold anything).
template <class T>
__global__ void k_nonfinite(const T* __restrict__ p, int64_t n, int64_t stride, int planes, int32_t* __restrict__ flag) {
  bool bad = false;
  for (int k = 0; k < planes; ++k)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      bad |= !isfinite(p[k * stride + i]);
  if (bad) atomicOr(flag, 1);
}
// the same check for each of a frame's planes at once (blockIdx.y = plane): flags[plane] |= 1
template <class T>
__global__ void k_nonfinite_planes(const T* __restrict__ p, int64_t n, int64_t stride, int32_t* __restrict__ flags) {
  const T* __restrict__ q = p + (int64_t)blockIdx.y * stride;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    bad |= !isfinite(q[i]);
  if (bad) atomicOr(flags + blockIdx.y, 1);
}
__global__ void k_window_nan(const int64_t* __restrict__ tot, int64_t n, int32_t* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    bad |= tot[i] >= tfg::kWindowNanMin;
  if (bad) atomicOr(flag, 1);
}

enum : uint8_t { kUnknown = 0, kOk = 1, kDirty = 2 };

// BMI input order (P_air, Hum_sp, P, T_air, uz) -> plane of a device forcing frame, on the host
constexpr int kBmiToPlane[5] = {F_PA, F_Q, F_P, F_T, F_UZ};
static_assert(kBmiToPlane[0] == tfg::kInputPlane[0] && kBmiToPlane[1] == tfg::kInputPlane[1] &&
                  kBmiToPlane[2] == tfg::kInputPlane[2] && kBmiToPlane[3] == tfg::kInputPlane[3] &&
                  kBmiToPlane[4] == tfg::kInputPlane[4],
              "k_forcing_regrid's plane of a source field is tfg_set_inputs' plane");

// tfg_selftest_powers: the fp64 engine's power rewrites (tfg_physics.hpp) and
// its exp / log / constant-divisor division (tfg_fastmath.hpp) on device, with
// the device libm's exp and log beside them
__global__ void k_selftest_powers(const double* __restrict__ x, double* __restrict__ y, int64_t n, int which) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    double r;
    switch (which) {
      case 0: r = tfg::pow4(v); break;
      case 1: r = tfg::pow1p5(v); break;
      case 2: r = tfg::root7(v); break;
      case 3: r = tfg_fm::exp_k(v); break;
      case 4: r = exp(v); break;
      case 5: r = tfg_fm::log_k(v); break;
      case 6: r = log(v); break;
      case 7: r = tfg_fm::div_k(v, 6.1121, 1.0 / 6.1121); break;
      case 9: r = tfg_fm::exp_kv(v); break;
      case 10: r = tfg_fm::fdiv(v, 7.3); break;
      case 11: r = tfg_fm::fdiv(7.3, v); break;
      case 12: r = tfg_fm::atan_q(v, 7.3); break;
      case 13: r = tfg_fm::atan_q(-7.3, v); break;
      default: r = tfg_fm::div_k(v, 3600.0, 1.0 / 3600.0); break;
    }
    y[i] = r;
  }
}

// ===========================================================================
// Host layer: what a handle owns
// ===========================================================================
namespace {

using tfg_host::Buf;

// The three kinds of memory the engine allocates (Buf's policies, tfg_hostbuf.hpp).
// tfg_selftest_powers aside, these are the file's only allocation and free calls.
struct DevMem {
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static int release(void* p) { return (int)hipFree(p); }
};
struct PinnedMem {
  static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static int release(void* p) { return (int)hipHostFree(p); }
};
struct MappedMem {  // pinned, device-mapped and coherent: kernels read and write it in place
  static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static int release(void* p) { return (int)hipHostFree(p); }
};

// A device buffer read as T: h->st + S_ALB * np, kernel arguments and `if (h->qc)` stay as with a raw pointer.
template <class T>
struct Dev : Buf<DevMem> {
  operator T*() const { return static_cast<T*>(ptr); }
  char* bytes() const { return static_cast<char*>(ptr); }  // for offsets in the engine's element size
};

// An event (timing off) and a non-blocking stream, created on first use and destroyed with their owner.
template <class T, hipError_t (*Destroy)(T)>
struct Owned {
  T v = nullptr;
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { if (v) (void)Destroy(v); }
  operator T() const { return v; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t create() { return v ? hipSuccess : hipEventCreateWithFlags(&v, hipEventDisableTiming); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return v ? hipSuccess : hipStreamCreateWithFlags(&v, hipStreamNonBlocking); }
};

// Two pinned slots for host data that is borrowed for one call only: the call
// copies it into the slot whose previous transfer has completed and queues the
// transfer from there (tfg_set_inputs, tfg_set_catchment_forcing and
// tfg_set_gridded_forcing share one ring, each slot with a device buffer of its own; tfg_step stages its
// uniforms through another, into d_u / d_u2).
struct StageRing {
  struct Slot {
    Buf<PinnedMem> host;
    Buf<DevMem> dev;
    Event done;   // the slot's transfer on the handle's stream
    Event done2;  // tfg_step only: its second copy, on the side stream
  };
  Slot slot[2];
  int next = 0;
  // The next slot, idle, with room for `bytes` (the old contents are not kept).
  hipError_t acquire(size_t bytes, bool with_dev, Slot** out) {
    Slot& s = slot[next];
    next ^= 1;
    hipError_t e = s.done.v ? hipEventSynchronize(s.done) : s.done.create();
    if (e == hipSuccess && s.done2.v) e = hipEventSynchronize(s.done2);
    if (e == hipSuccess) e = (hipError_t)s.host.reserve(bytes);
    if (e == hipSuccess && with_dev) e = (hipError_t)s.dev.reserve(bytes);
    *out = &s;
    return e;
  }
  static hipError_t commit(Slot& s, hipStream_t stream) { return hipEventRecord(s.done, stream); }
};

// A pinned, device-mapped host block that kernels read their inputs from and
// write their outputs and release flags to, zeroed when (re)allocated; the
// launches that use it are numbered from 1, a fresh flag's 0 never among them.
struct MappedBlock {
  Buf<MappedMem> mem;
  char* dev = nullptr;
  uint32_t seq = 0;
  char* host() const { return static_cast<char*>(mem.ptr); }
  // Callers ask mem.cap < bytes first and wait for the launches that still use the block.
  hipError_t reserve(size_t bytes) {
    dev = nullptr;
    seq = 0;
    if (const int e = mem.reserve(bytes)) return (hipError_t)e;
    std::memset(mem.ptr, 0, bytes);
    const hipError_t e = hipHostGetDevicePointer((void**)&dev, mem.ptr, 0);
    if (e != hipSuccess) (void)mem.reset();
    return e;
  }
  uint32_t next_seq() { return ++seq ? seq : ++seq; }
};

}  // namespace

// Every resource is an owning member: `delete h` releases them all, in reverse
// order of declaration (the streams last), and an empty handle makes no HIP call.
struct tfg_handle {
  Stream own_stream, side;       // the handle's own stream, and a split launch's second part's (tfg_set_split)
  hipStream_t stream = nullptr;  // own_stream, or the caller's (tfg_set_stream)
  int device = 0, engine = TFG_F32;
  int64_t ny = 0, nx = 0, n = 0, n_pad = 0;
  int n_frames = 1, hist_depth = 1, n_catch = 1, ring_len = 72;
  size_t rsz = 4;
  DevParams dp{};
  Dev<void> forc, stat;
  Dev<void> lwsw;                // [2][n_pad] R, not read by the physics
  Dev<float> geo;                // fast engine: [5][n_pad] f32 + [2][n_pad] f64 solar geometry; exact: [kStaticPlanes][n_pad] f64 CellStatic
                                 // (elev, cos_leq, sin_leq, dlon, tan_eq, cos_dlon, sin_dlon)
  bool geo_dirty = true;
  Dev<int32_t> catch_id;         // [n_pad], allocated (zeroed) by the first TFG_ST_CATCH_ID set
  Dev<double> st;
  Dev<int64_t> tot;
  Dev<int32_t> ring;
  Dev<void> hist;
  Dev<double> diag;              // [n_catch][6]
  Dev<double> slab;              // [max_blocks][n_catch][6]
  // The history readers' scratch (tfg_catchment_series, tfg_band_series, tfg_coarse_series): one reader runs
  // at a time, on `stream`, so they share it; each call reserves what it needs (reserve_idle)
  Dev<double> rd_part_sum;       // the workgroups' fp64 partials
  Dev<int32_t> rd_part_int;      // their int32 partials (counts; the band series' cells after them)
  Dev<double> rd_out_sum;        // a host call's fp64 result on the device
  Dev<int64_t> rd_out_int;       // its int64 results (counts, then cells)
  // tfg_coarse_series: the tables of the last grid (coarse_plan), kept while the grid's bytes stay the same
  Dev<int32_t> coarse_tab;
  tfg_forcing_grid coarse_grid{};  // the grid coarse_tab holds (method and pad zeroed), while coarse_valid
  CoarsePlan coarse;
  bool coarse_valid = false;
  Dev<float> d_diurnal;
  Dev<int32_t> d_flag;
  // tfg_step's staged steps: [nsteps] tfg_uniforms, then the [nsteps] StepAddr
  // records of the same steps (step_table, stage_bytes); d_u2 and u_ring's slots alike
  Dev<tfg_uniforms> d_u;
  StageRing u_ring;
  Dev<void> staging;             // upload / download's conversion scratch
  int max_blocks = 2048;
  int fuse = 24;
  bool depths_derived = false;
  bool slope_invalid = false;
  bool initialised = false;
  bool tot_dirty = false;        // window slots set through TFG_ST_WINDOW
  // scratch and halo rows, allocated on first use
  Dev<double> wtmp;              // [n_pad] f64 scratch for window I/O
  Dev<double> halo;              // [2][nx] f64 DEM halo rows (tfg_terrain_from_dem)
  Dev<double> flow_halo;         // [2 sides][2][nx] f64 ice-flow halo rows (s, H)
  Dev<double> flow_edges;        // [2 rows][2][nx] f64 this shard's edge rows
  Dev<double> flow_red;          // f64 per-workgroup maxima of k_ice_flow<R, true>
  double flow_gamma = 0.0;       // 2A/(n+2) (rho_ice g)^n, n = 3 [m^-3 yr^-1]
  // optional lateral conduction: Qc plane (engine type) added to Q_sum while qc_on
  Dev<void> qc;                  // [n_pad] R, allocated (zeroed) on first use
  bool qc_on = false;
  Dev<double> cond_halo;         // [2 sides][4][nx] f64 halo rows (T_snow, h_snow, T_ice, h_ice)
  Dev<double> cond_edges;        // [2 rows][4][nx] f64 this shard's edge rows
  double inv_cs = 0.0, inv_ci = 0.0, h_active = 0.0;  // 1/(rho_s Cp_s), 1/(rho_i Cp_i h_al), h_al
  // tfg_set_inputs, tfg_set_catchment_forcing and tfg_set_gridded_forcing: host sources go through this ring
  StageRing in_ring;
  // tfg_get_outputs: device gather buffer + pinned host buffer
  Dev<void> out_d;
  Buf<PinnedMem> out_h;
  // tfg_update: one block (inputs | uniforms | outputs | flags) that the
  // kernels read and write directly through its device mapping
  MappedBlock io;
  int64_t last_hist = 0;
  // Finite-data tracking for the fp32 engine's two step forms (tfg_physics.hpp,
  // "Missing data"): a launch runs the clean form only when everything it reads
  // is known to be finite.  kUnknown: written by a path that did not check it;
  // kDirty: checked, holds a NaN or an infinity.
  std::vector<uint8_t> plane_state;  // [n_frames][kNumForc] forcing planes
  std::vector<int> chk_frames;       // choose_form's scratch list of frames to check
  uint8_t state_state = 1;           // fp64 state planes and the snowfall window
  uint8_t elev_state = 1;            // the elevation raster (the fp32 flux reads it unguarded)
  uint8_t qc_state = 1;              // the Qc plane while the conduction term is on
  int state_recheck = 0;             // launches before a dirty state is checked again
  int64_t ns_launches = 0;           // launches that ran the NaN-safe form (tfg_nan_safe_launches)
  bool force_ns = false;             // tfg_set_step_form(TFG_FORM_NAN_SAFE): every launch NaN-safe
  bool flux_f64 = false;             // tfg_set_flux(TFG_FLUX_F64): the fp32 engine's fp64-flux form
  // Split launches (tfg_set_split): the side stream's copy of the step
  // uniforms, and the events that order it against the handle's stream
  int split_mode = TFG_SPLIT_AUTO;
  Event side_fork, side_join;
  Dev<tfg_uniforms> d_u2;
  bool side_busy = false;   // the side stream holds launches the handle's stream is not yet ordered after
  bool side_stale = true;   // the handle's stream holds work the side stream's next launch must follow
  std::string err;
};

namespace {

int fail(tfg_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_err = msg;
  return code;
}

#define HIPCHK(h, call)                                                                  \
  do {                                                                                   \
    const hipError_t e_ = (hipError_t)(call); /* Buf passes HIP's codes on as int */    \
    if (e_ != hipSuccess)                                                                \
      return fail((h), TFG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

size_t dtype_size(int dt) { return dt == TFG_F64 ? 8 : 4; }

// Run f(Tag<float>) or f(Tag<double>) by a TFG_F32 / TFG_F64 dtype (the
// handle's engine type, mostly): one spelling of a launch for both instances
// of a kernel.  by_types: the same over a pair of dtypes.
template <class T> struct Tag { using type = T; };
template <class F>
decltype(auto) by_type(int dtype, F&& f) { return dtype == TFG_F32 ? f(Tag<float>{}) : f(Tag<double>{}); }
template <class F>
decltype(auto) by_types(int dt_a, int dt_b, F&& f) {
  return by_type(dt_a, [&](auto a) { return by_type(dt_b, [&](auto b) { return f(a, b); }); });
}

// A buffer allocated on first use and zero-filled then (a later call finds it large enough).
template <class B>
int reserve_zeroed(tfg_handle* h, B& b, size_t bytes) {
  if (bytes <= b.cap) return TFG_OK;
  HIPCHK(h, b.reserve(bytes));
  HIPCHK(h, hipMemsetAsync(b.ptr, 0, bytes, h->stream));
  return TFG_OK;
}
int ensure_qc(tfg_handle* h) { return reserve_zeroed(h, h->qc, (size_t)h->n_pad * h->rsz); }

// At least `bytes` of a buffer that work queued on the handle's stream may still use (tfg_hostbuf.hpp's rule):
// growing releases the old allocation, so the stream is drained first; nothing else waits.
template <class B>
hipError_t reserve_idle(tfg_handle* h, B& b, size_t bytes) {
  if (bytes <= b.cap) return hipSuccess;
  const hipError_t e = b.ptr ? hipStreamSynchronize(h->stream) : hipSuccess;
  return e != hipSuccess ? e : (hipError_t)b.reserve(bytes);
}

// Split launches (include/tfg.h tfg_set_split).  The parts are whole 256-cell
// chunks; AUTO splits grids of one to 64 rounds of the resident workgroups.
bool split_active(const tfg_handle* h) {
  if (h->engine != TFG_F32 || h->split_mode == TFG_SPLIT_OFF) return false;
  if (h->split_mode == TFG_SPLIT_ON) return h->n_pad >= 2 * kBlock;
  return h->n >= ((int64_t)1 << 18) && h->n <= ((int64_t)1 << 24);
}
// The handle's stream after the side stream's launches so far (no host wait).
int join_side(tfg_handle* h) {
  if (!h->side_busy) return TFG_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->side_join, h->side));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->side_join, 0));
  h->side_busy = false;
  return TFG_OK;
}
// The side stream after the handle's stream's work so far: only when that
// holds something other than the first parts' launches (a field set, the
// window totals, ...), so consecutive tfg_step calls leave the streams free.
int fork_side(tfg_handle* h) {
  if (!h->side_stale) return TFG_OK;
  HIPCHK(h, hipEventRecord(h->side_fork, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->side, h->side_fork, 0));
  h->side_stale = false;
  return TFG_OK;
}
// Every API call but tfg_step: order the handle's stream after the side's
// launches, and have the side's next launch follow what the call queues.
int api_sync(tfg_handle* h) {
  if (!h) return TFG_OK;
  h->side_stale = true;
  return join_side(h);
}
int ensure_side(tfg_handle* h) {
  if (h->side.v) return TFG_OK;
  HIPCHK(h, h->side.create());
  HIPCHK(h, h->side_fork.create());
  HIPCHK(h, h->side_join.create());
  h->side_stale = true;
  return TFG_OK;
}

// k_forcing_expand's cells per lane: 16-byte stores (4 float / 2 double cells),
// or with TFG_FORCING_CELLS=1 in the environment one cell per lane -- the
// form it was measured against (tests/diagnostics/catchment_forcing_timing.py;
// read at every call, so one process can time both)
bool forcing_wide() {
  const char* e = std::getenv("TFG_FORCING_CELLS");
  return !(e && e[0] == '1' && e[1] == 0);
}

int grid_for(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 8192); }

// dst (type dt) <- src (type st), both on the device, the two types different
int convert(tfg_handle* h, void* dst, int dt, const void* src, int st, int64_t n) {
  if (!((dt == TFG_F32 && st == TFG_F64) || (dt == TFG_F64 && st == TFG_F32)))
    return fail(h, TFG_ERR_ARG, "unsupported dtype conversion");
  by_types(dt, st, [&](auto d, auto s) {
    using D = typename decltype(d)::type;
    using S = typename decltype(s)::type;
    if constexpr (!std::is_same_v<D, S>)
      hipLaunchKernelGGL((k_convert<D, S>), grid_for(n), 256, 0, h->stream, (D*)dst, (const S*)src, n);
  });
  HIPCHK(h, hipGetLastError());
  return TFG_OK;
}

// copy n elements of type st (host/device) into device buffer dst of type dt
int upload(tfg_handle* h, void* dst, int dt, const void* src, int st, int64_t n, int on_dev) {
  if (n <= 0) return TFG_OK;
  const size_t sbytes = (size_t)n * dtype_size(st);
  if (dt == st) {
    HIPCHK(h, hipMemcpyAsync(dst, src, sbytes, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  } else {
    if (!on_dev) {
      HIPCHK(h, h->staging.reserve(sbytes));
      HIPCHK(h, hipMemcpyAsync(h->staging, src, sbytes, hipMemcpyHostToDevice, h->stream));
      src = h->staging;
    }
    if (int rc = convert(h, dst, dt, src, st, n)) return rc;
  }
  if (!on_dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

// Whether the kernel(s) `launch` queues on the handle's stream set d_flag[0] (synchronous).
template <class Launch>
int read_flag(tfg_handle* h, bool* set, Launch&& launch) {
  HIPCHK(h, hipMemsetAsync(h->d_flag, 0, 4, h->stream));
  launch();
  HIPCHK(h, hipGetLastError());
  int32_t flag = 0;
  HIPCHK(h, hipMemcpyAsync(&flag, h->d_flag, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *set = flag != 0;
  return TFG_OK;
}

// kOk when every value of n cells at device pointer p is finite, kDirty otherwise (synchronous).
int check_finite(tfg_handle* h, const void* p, int dtype, int64_t n, uint8_t* out) {
  bool bad = false;
  int rc = read_flag(h, &bad, [&] {
    by_type(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((k_nonfinite<T>), grid_for(n), 256, 0, h->stream, (const T*)p, n, (int64_t)0, 1, h->d_flag);
    });
  });
  if (rc == TFG_OK) *out = bad ? kDirty : kOk;
  return rc;
}

// Finite-data status of the n cells just written at device pointer p
// (tfg_handle::plane_state; the fp32 engine only).  A device source keeps the
// set stream-ordered: kUnknown, checked before a launch long enough to pay for
// it (choose_form).  A host source is checked now (its upload was synchronous).
// sticky: `state` covers more than this plane (state_state), so only a bad one shows.
int note_written(tfg_handle* h, const void* p, int dtype, int64_t n, bool on_dev, uint8_t* state, bool sticky = false) {
  if (h->engine != TFG_F32) return TFG_OK;
  uint8_t st = kUnknown;
  if (!on_dev)
    if (int rc = check_finite(h, p, dtype, n, &st)) return rc;
  if (!sticky || st != kOk) *state = st;
  return TFG_OK;
}

// The same check on host values as the fp32 engine will hold them (the BMI
// inputs of tfg_update / tfg_set_inputs, a table's rows): finite after the
// conversion (a finite double beyond FLT_MAX becomes inf in the frame).
template <class T>
uint8_t host_finite_as_f32(const T* p, int64_t n) {
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) bad |= !std::isfinite((float)p[i]);
  return bad ? kDirty : kOk;
}

int download(tfg_handle* h, void* dst, int dt, const void* src, int st, int64_t n, int on_dev) {
  if (n <= 0) return TFG_OK;
  const size_t dbytes = (size_t)n * dtype_size(dt);
  const void* dsrc = src;
  if (dt != st) {
    void* conv = dst;
    if (!on_dev) {
      HIPCHK(h, h->staging.reserve(dbytes));
      conv = h->staging;
    }
    if (int rc = convert(h, conv, dt, src, st, n)) return rc;
    if (on_dev) return TFG_OK;
    dsrc = conv;
  }
  HIPCHK(h, hipMemcpyAsync(dst, dsrc, dbytes, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  if (!on_dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

void derive_params(const tfg_params& q, DevParams& p) {
  std::memset(&p, 0, sizeof(p));
  const double pi = 3.141592653589793;
  p.dt = q.dt;
  p.da_m2 = q.da_m2;
  p.T_rs = q.T_rain_snow;
  p.dust = q.dust_atten;
  p.F = q.canopy_factor;
  p.one_minus_F_172 = (1.0 - q.canopy_factor) * 1.72;
  p.cloud_term = 1.0 + (0.22 * (q.cloud_factor * q.cloud_factor));
  p.rho_snow_Cp_snow = q.rho_snow * q.Cp_snow;
  p.rho_air_Cp_air = q.rho_air * q.Cp_air;
  p.rho_air_Lv = q.rho_air * q.Lv;
  p.rho_H2O_Lf = q.rho_H2O * q.Lf;
  p.inv_rho_H2O_Lf = 1.0 / p.rho_H2O_Lf;
  p.lhc_100_p0 = q.latent_heat_constant * 100.0 / q.sea_level_p0;
  p.inv_6p11 = 1.0 / (0.611 * 10.0);
  p.negM_g = -q.M_mass_air * q.g;
  p.R = q.uni_gas_const;
  p.eps = q.eps;
  p.one_minus_eps = 1.0 - q.eps;
  p.z = 10.0;
  p.gz = q.g * 10.0;
  p.kappa = q.kappa;
  p.z0 = q.z0_air;
  p.sigma = q.sigma;
  p.em_surf_sigma = q.em_surf * q.sigma;
  p.one_minus_em_surf = 1.0 - q.em_surf;
  p.negM_g_R = -q.M_mass_air * q.g / q.uni_gas_const;
  p.T0 = q.T0;
  p.ws = q.rho_H2O / q.rho_snow;
  p.wi = q.rho_H2O / q.rho_ice;
  p.days_per_dt = q.dt / 86400.0;
  p.pi_over_180 = pi / 180.0;
  p.c180_over_pi = 180.0 / pi;
  p.sin_lat = q.sin_lat;  // numpy values from the host (the reference computes them with numpy)
  p.cos_lat = q.cos_lat;
  {
    // Ecci = max(((rho_ice*Cp_ice)*h_active_layer)*del_T, 0), del_T = T0 - 0  (:394-395)
    const double e = (q.rho_ice * q.Cp_ice) * q.h_active_layer * (q.T0 - 0.0);
    p.Ecci0 = (e >= 0.0 || e != e) ? e : 0.0;
  }
  p.omega = tfg::kOmega;  // (360 / 24) * (pi / 180)
  p.half_pi = pi / 2.0;
  p.twopi = 2.0 * pi;
  p.qscale = 68719476736.0;  // 2^36
  p.thr_q = (int64_t)std::ceil(0.03 * 68719476736.0);
  p.satterlund = q.satterlund;
  p.ring_len = q.ring_len;
  p.inv_dt = 1.0 / q.dt;
  p.inv_dt_rhoLf = 1.0 / (q.dt * p.rho_H2O_Lf);
  p.c_sm3600 = 3600.0 / (q.dt * p.rho_H2O_Lf);
  p.dt3600 = q.dt * 3600.0;
  {
    float t = (float)q.T_rain_snow;  // largest float <= T_rain_snow
    if ((double)t > q.T_rain_snow) t = std::nextafter(t, -INFINITY);
    p.f_T_rs_dn = t;
  }
  p.f_eps100 = (float)(100.0 * q.eps);
  p.f_ome100 = (float)(100.0 * (1.0 - q.eps));
  p.f_gz = (float)p.gz;
  p.f_z = 10.0f;
  p.f_k2 = (float)((q.kappa / std::log(2.0)) * (q.kappa / std::log(2.0)));
  p.f_rho_air_Cp_air = (float)p.rho_air_Cp_air;
  p.f_qe = (float)(p.rho_air_Lv * q.latent_heat_constant * 100.0 / q.sea_level_p0);
  p.f_dust = (float)q.dust_atten;
  p.f_1pdust = (float)(1.0 + q.dust_atten);
  p.f_em_surf_sigma = (float)p.em_surf_sigma;
  p.f_qfac = (float)(q.dt * p.ws * p.qscale);
  p.f_dt = (float)q.dt;
  p.f_T0 = (float)q.T0;
  p.f_c_eccs = (float)(p.rho_snow_Cp_snow * q.dt * p.ws);
  p.inv_z0 = 1.0 / q.z0_air;
  {
    const int k = (int)std::lround(std::log2(0.7 * p.z / q.z0_air));  // (z - h)/z0 near 2^k for h ~ 0.3 z
    p.f_inv_z0s = (float)std::ldexp(1.0 / q.z0_air, -k);
    p.f_l2k2 = (float)(2 * k);
    p.f_l2kk = (float)(k * k);
    p.f_l2min = (float)std::ldexp(0.01, -k);
  }
  p.f_em_sc = 102.4f;  // 0.1 * 2^10
  p.f_ccFs = (float)(p.one_minus_F_172 * p.cloud_term * std::exp2(-10.0 / 7.0));
  p.f_Fm1 = (float)(q.canopy_factor - 1.0);
  p.d_eps100 = 100.0 * q.eps;
  p.d_ome100 = 100.0 * (1.0 - q.eps);
  p.d_k2 = (q.kappa / std::log(2.0)) * (q.kappa / std::log(2.0));
  p.d_l2k = (double)p.f_l2k2 * 0.5;
  p.d_l2kk = (double)p.f_l2kk;
  // exp(c) of the flux form's lhc / p0 = exp(c) exp(y - c) (tfg_fm::exp_near)
  p.d_qe = p.rho_air_Lv * q.latent_heat_constant * 100.0 / q.sea_level_p0 * std::exp(tfg_fm::kP0Center);
  p.d_es_k = q.satterlund ? 2353.0 * std::log(10.0) : 17.3 * 237.3;
  p.d_es_c = q.satterlund ? 273.15 : 237.3;
}

void* field_ptr(tfg_handle* h, int field, int index, int* dtype) {
  const int64_t np = h->n_pad;
  const size_t rs = h->rsz;
  char* f = h->forc.bytes();
  char* hs = h->hist.bytes();
  switch (field) {
    case TFG_IN_LW_IN: *dtype = h->engine; return h->lwsw.bytes();
    case TFG_IN_SW_IN: *dtype = h->engine; return h->lwsw.bytes() + np * rs;
    case TFG_IN_P: *dtype = h->engine; return f + ((int64_t)index * kNumForc + F_P) * np * rs;
    case TFG_IN_T_AIR: *dtype = h->engine; return f + ((int64_t)index * kNumForc + F_T) * np * rs;
    case TFG_IN_HUM_SP: *dtype = h->engine; return f + ((int64_t)index * kNumForc + F_Q) * np * rs;
    case TFG_IN_P_AIR: *dtype = h->engine; return f + ((int64_t)index * kNumForc + F_PA) * np * rs;
    case TFG_IN_UZ: *dtype = h->engine; return f + ((int64_t)index * kNumForc + F_UZ) * np * rs;
    case TFG_OUT_H_SNOW: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_HSNOW) * np * rs;
    case TFG_OUT_SM: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_SM) * np * rs;
    case TFG_OUT_H_ICE: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_HICE) * np * rs;
    case TFG_OUT_IM: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_IM) * np * rs;
    case TFG_OUT_M_TOTAL: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_MTOT) * np * rs;
    case TFG_OUT_RH: *dtype = h->engine; return hs + ((int64_t)index * kNumHist + H_RH) * np * rs;
    case TFG_OUT_H_SWE: *dtype = TFG_F64; return h->st + S_HSWE * np;
    case TFG_OUT_H_IWE: *dtype = TFG_F64; return h->st + S_HIWE * np;
    case TFG_ST_ELEV: *dtype = h->engine; return h->stat.bytes();
    case TFG_ST_SLOPE: *dtype = h->engine; return h->stat.bytes() + np * rs;
    case TFG_ST_ASPECT: *dtype = h->engine; return h->stat.bytes() + 2 * np * rs;
    case TFG_ST_CATCH_ID: *dtype = TFG_I32; return h->catch_id;
    case TFG_ST_ECCS: *dtype = TFG_F64; return h->st + S_ECCS * np;
    case TFG_ST_ECCI: *dtype = TFG_F64; return h->st + S_ECCI * np;
    case TFG_ST_ALBEDO: *dtype = h->engine == TFG_F32 ? TFG_F32 : TFG_F64; return h->st + S_ALB * np;  // fp32 engine: fp32
    case TFG_ST_NDAYS: *dtype = TFG_F64; return h->st + S_N * np;
    default: return nullptr;
  }
}

bool is_frame_field(int f) { return f == TFG_IN_P || f == TFG_IN_T_AIR || f == TFG_IN_HUM_SP || f == TFG_IN_P_AIR || f == TFG_IN_UZ; }
bool is_hist_field(int f) { return f == TFG_OUT_H_SNOW || f == TFG_OUT_SM || f == TFG_OUT_H_ICE || f == TFG_OUT_IM || f == TFG_OUT_M_TOTAL || f == TFG_OUT_RH; }

// What a reader of the output history is given: `nslots` slots of one field from slot `hist0`, following the ring.
struct HistWindow {
  const void* plane = nullptr;  // slot 0's plane of the field, engine type
  int64_t stride = 0;           // elements from a slot's plane to the next slot's
  int depth = 0, hist0 = 0, nslots = 0;
  // for (int j0 = 0; j0 < w.nslots; j0 += B): the batch of at most B slots from the window's slot j0, which is the
  // ring's slot slot0.
  struct Batch { int nb, slot0; };
  Batch batch(int j0, int B) const { return {std::min(B, nslots - j0), (hist0 + j0) % depth}; }
};
// The window of a call's arguments, or TFG_ERR_ARG under the caller's name.
int hist_window(tfg_handle* h, const char* who, int field, int hist0, int nslots, HistWindow* w) {
  auto bad = [&](const std::string& what) { return fail(h, TFG_ERR_ARG, std::string(who) + ": " + what); };
  if (!is_hist_field(field)) return bad("field " + std::to_string(field) + " is not a history field (h_snow, SM, h_ice, IM, M_total, RH)");
  if (hist0 < 0 || hist0 >= h->hist_depth) return bad("first history slot out of range");
  if (nslots < 1 || nslots > h->hist_depth) return bad("slot count outside 1..hist_depth");
  int fdt = 0;
  *w = {field_ptr(h, field, 0, &fdt), (int64_t)kNumHist * h->n_pad, h->hist_depth, hist0, nslots};
  return TFG_OK;
}

// tfg_update's single-step launch (KArgs::io_*); empty for every other launch
struct IoArgs {
  const void* in = nullptr;
  double* out = nullptr;
  uint32_t* flag = nullptr;
  uint32_t seq = 0;
  uint8_t in_state = kUnknown;  // the inputs' finite-data status (tfg_handle::plane_state)
};

// One part of a split launch (launch_steps): cells [c0, c0 + cells) of the
// plane stride, n_valid of them grid cells, on `stream` with its own uniforms;
// its workgroups fold into slab rows from slab_row0.
struct Part {
  int64_t c0, cells, n_valid, slab_row0;
  hipStream_t stream;
};

// The KArgs of K steps over the handle's whole plane stride (a part of a split launch narrows them).
KArgs step_args(const tfg_handle* h, int K, const IoArgs& io) {
  KArgs a;
  a.p = h->dp;
  a.K = K;
  a.io_in = io.in;
  a.io_out = io.out;
  a.io_flag = io.flag;
  a.io_seq = io.seq;
  a.n_catch = h->n_catch;
  a.n = h->n;
  a.n_pad = h->n_pad;
  a.n_step = h->n_pad;
  return a;
}

template <class R, bool EXACT>
int launch_fused(tfg_handle* h, const tfg_uniforms* d_u, const StepAddr* d_t, int K, int blocks, size_t lds,
                 const IoArgs& io, bool ns, const Part* part = nullptr) {
  const hipStream_t stream = part ? part->stream : h->stream;
  KArgs a = step_args(h, K, io);
  if (part) {
    a.n = part->n_valid;
    a.n_step = part->cells;
  }
  // a part's buffers start at its first cell in every plane (the planes keep
  // their stride); the kernel corrects its two mixed-width views by c0
  const int64_t c0 = part ? part->c0 : 0;
  a.part_c0 = c0;
  const size_t rb = (size_t)c0 * h->rsz;
  const FusedBufs fb = {d_u, d_t, h->forc.bytes() + rb, h->stat.bytes() + rb, h->geo + c0,
                        h->catch_id ? h->catch_id + c0 : nullptr, h->st + c0, h->tot + c0, h->ring + c0,
                        h->hist.bytes() + rb, h->slab + (part ? part->slab_row0 : 0) * h->n_catch * 6,
                        h->qc ? h->qc.bytes() + rb : nullptr};
  const bool rd = !h->depths_derived;
  const bool ct = h->catch_id != nullptr;
  if constexpr (EXACT) {  // the fp64 engine's instantiations live in tfg_fused_f64.hip
    HIPCHK(h, launch_fused_exact(a, fb, rd, ct, h->qc_on, blocks, lds, stream));
    return TFG_OK;
  } else {
    // the form's instantiations live in its own unit (tfg_fused.hpp, launch_fused_fast)
    const bool sat = h->dp.satterlund != 0;
    hipError_t e;
    if (h->flux_f64) e = sat ? launch_fused_fast<true, true>(a, fb, rd, ct, h->qc_on, ns, blocks, lds, stream)
                             : launch_fused_fast<true, false>(a, fb, rd, ct, h->qc_on, ns, blocks, lds, stream);
    else e = sat ? launch_fused_fast<false, true>(a, fb, rd, ct, h->qc_on, ns, blocks, lds, stream)
                 : launch_fused_fast<false, false>(a, fb, rd, ct, h->qc_on, ns, blocks, lds, stream);
    HIPCHK(h, e);
    return TFG_OK;
  }
}

}  // namespace

// the default form of the fp32 engine's k_fused (Brutsaert, fp32 fluxes) is compiled in this unit
template hipError_t tfg_kern::launch_fused_fast<false, false>(const KArgs&, const FusedBufs&, bool, bool, bool, bool, int,
                                                              size_t, hipStream_t);

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int tfg_abi_version(void) { return TFG_ABI_VERSION; }

#ifndef TFG_SRC_HASH
#define TFG_SRC_HASH "unknown"
#endif
// build() (__graft_entry__.py) passes the sha256 of the sources and flags; it
// finds this string in the built library to decide whether to recompile.  Host
// side only: in the device code it would make the code objects (whose sha256
// keys the PMC provenance in bench.py) change with every source edit.
#define TFG_STR2(x) #x
#define TFG_STR(x) TFG_STR2(x)
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((used)) static const char tfg_build_tag[] =
    "libtfg abi=" TFG_STR(TFG_ABI_VERSION) " arch=gfx950 (hipcc) tfg-src-sha256=" TFG_SRC_HASH
    "; kernels: k_fused<float|double,exact|fast,...>, k_cell, k_cell_run, k_cell_many, k_diag_reduce, k_catch_series, k_band_series, k_forcing_expand, k_forcing_regrid, k_fill_synthetic";

const char* tfg_build_info(void) { return tfg_build_tag; }
#else
const char* tfg_build_info(void);
#endif

int tfg_device_count(int* count) {
  if (!count) return fail(nullptr, TFG_ERR_ARG, "null count");
  HIPCHK(nullptr, hipGetDeviceCount(count));
  return TFG_OK;
}

// Plane-stride skew of large shards (tfg_create), a multiple of the 256-cell chunk.
constexpr int64_t kPlaneSkew = 512;

int tfg_create(const tfg_params* p, int64_t ny, int64_t nx, int engine, int device, int n_frames,
               int hist_depth, int n_catch, tfg_handle** out) {
  if (!p || !out) return fail(nullptr, TFG_ERR_ARG, "null params/out");
  *out = nullptr;
  if (ny <= 0 || nx <= 0) return fail(nullptr, TFG_ERR_ARG, "grid must have ny, nx >= 1");
  if (ny > (1ll << 31) || nx > (1ll << 31))  // before forming ny*nx
    return fail(nullptr, TFG_ERR_ARG, "shard too large: ny and nx must stay below 2^31");
  if (engine != TFG_F32 && engine != TFG_F64) return fail(nullptr, TFG_ERR_ARG, "engine must be TFG_F32 or TFG_F64");
  if (n_frames < 1 || hist_depth < 1 || n_catch < 1) return fail(nullptr, TFG_ERR_ARG, "n_frames, hist_depth, n_catch must be >= 1");
  if (n_catch > 512) return fail(nullptr, TFG_ERR_ARG, "n_catch > 512 not supported");
  if (p->ring_len < 1) return fail(nullptr, TFG_ERR_ARG, "ring_len must be >= 1");
  if (!(p->dt > 0)) return fail(nullptr, TFG_ERR_ARG, "dt must be > 0");
  // derive_params takes log2(z / z0_air) and squares its rounding (the roughness
  // log's scaling): a z0_air that is zero, negative, NaN or infinite has none
  if (!(p->z0_air > 0.0 && p->z0_air < INFINITY)) return fail(nullptr, TFG_ERR_ARG, "z0_air must be finite and > 0");
  tfg_handle* h = new (std::nothrow) tfg_handle();
  if (!h) return fail(nullptr, TFG_ERR_ARG, "out of host memory");
  auto bail = [&](int rc) {
    g_err = h->err;
    tfg_destroy(h);
    return rc;
  };
  h->device = device;
  h->engine = engine;
  h->rsz = dtype_size(engine);
  h->ny = ny;
  h->nx = nx;
  h->n = ny * nx;
  h->n_pad = round_up(h->n, 64);
  // Plane stride n_pad = round_up(n, 64) + kPlaneSkew cells for shards of 2^20
  // cells or more, so that the planes of a power-of-two shard do not sit at
  // power-of-two distances.  With the plain stride the streaming rate depended
  // on where the allocator put the buffers: 105-115 G cell-updates/s over fresh
  // allocations of one 4096^2 shard in one process, 113.8-116.0 with 512 cells
  // (2 KB) of skew; 1024 x 8192: 111.9-114.1 against 113.7-115.2; 8192^2:
  // 116.4-117.4 against 117.2-117.5 (tests/diagnostics/alloc_variance.py,
  // HISTORY.md section 5).
  h->n_pad += h->n_pad >= ((int64_t)1 << 20) ? kPlaneSkew : 0;
  if (h->n_pad * 8 >= (int64_t)1 << 32) {
    h->err = "shard too large: ny*nx must stay below 2^29 cells per device (32-bit field offsets)";
    g_err = h->err;
    delete h;
    return TFG_ERR_ARG;
  }
  h->n_frames = n_frames;
  h->hist_depth = hist_depth;
  h->n_catch = n_catch;
  h->ring_len = p->ring_len;
  derive_params(*p, h->dp);
  {
    const double rg = p->rho_ice * p->g;  // Glen's law n = 3: Gamma = 2A/5 (rho_ice g)^3
    h->flow_gamma = 2.0 * p->glens_A / 5.0 * (rg * rg * rg);
    h->inv_cs = 1.0 / (p->rho_snow * p->Cp_snow);
    h->inv_ci = 1.0 / ((p->rho_ice * p->Cp_ice) * p->h_active_layer);
    h->h_active = p->h_active_layer;
  }
  if (hipSetDevice(device) != hipSuccess) { h->err = "hipSetDevice failed"; return bail(TFG_ERR_HIP); }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { h->err = "hipGetDeviceProperties failed"; return bail(TFG_ERR_HIP); }
  // 512 workgroups per CU: each thread walks ~2 cells at 8192^2.  Freshly
  // dispatched workgroups start their per-cell state loads at staggered times,
  // which hides the latency bubble at the start of every cell; measured
  // +9 % for 128 per CU over 8 (round 1), and with the two-step prefetch
  // +0.6 % for 512 over 128 at 8192^2, +0.6 % on the 4096 x 8192 shard, even
  // at 4096^2 (where the chunk count caps it at 256 per CU; HISTORY.md
  // section 5).  The per-workgroup diagnostic slab is kept under 256 MiB for
  // large catchment counts: 65536 workgroups at config 5's 43 catchments
  // (135 MB), +1.2 % on its slab against the 16384 a 64 MiB cap gave.
  h->max_blocks = std::max(256, prop.multiProcessorCount * 512);
  h->max_blocks = (int)std::max<int64_t>(256, std::min<int64_t>(h->max_blocks, (256ll << 20) / ((int64_t)n_catch * 6 * 8)));
  // a power of two: with many catchments a slab-capped odd count (31775 at 44
  // catchments) measured 10 % slower than 32768 or 16384 (A/B, same box)
  while (h->max_blocks & (h->max_blocks - 1)) h->max_blocks &= h->max_blocks - 1;
  // no more workgroups (slab rows) than the grid has chunks: a one-cell BMI
  // handle keeps one row, not 32768 (NextGen may hold thousands of handles)
  h->max_blocks = (int)std::min<int64_t>(h->max_blocks, (h->n_pad / kCellsPerThread + kBlock - 1) / kBlock);
  if (h->own_stream.create() != hipSuccess) { h->err = "stream create failed"; return bail(TFG_ERR_HIP); }
  h->stream = h->own_stream;
  const int64_t np = h->n_pad;
  const size_t rs = h->rsz;
  struct A { Buf<DevMem>* b; size_t bytes; } allocs[] = {
      {&h->forc, (size_t)n_frames * kNumForc * np * rs},
      {&h->stat, 3 * (size_t)np * rs},
      {&h->lwsw, 2 * (size_t)np * rs},
      {&h->geo, engine == TFG_F32 ? (size_t)np * (tfg::kGeoF * 4 + 2 * 8) : (size_t)np * tfg::kStaticPlanes * 8},
      {&h->st, (size_t)kNumState * np * 8},
      {&h->tot, (size_t)np * 8},
      {&h->ring, (size_t)p->ring_len * np * 4},
      {&h->hist, (size_t)hist_depth * kNumHist * np * rs},
      {&h->diag, (size_t)n_catch * 6 * 8},
      {&h->slab, (size_t)h->max_blocks * n_catch * 6 * 8},
      {&h->d_flag, (size_t)n_frames * kNumForc * 4},  // a flag per forcing plane (choose_form)
  };
  for (auto& a : allocs) {
    const hipError_t e = (hipError_t)a.b->reserve(a.bytes);
    if (e != hipSuccess) {
      h->err = std::string("hipMalloc(") + std::to_string(a.bytes) + " B) failed: " + hipGetErrorString(e);
      return bail(TFG_ERR_HIP);
    }
    if (hipMemsetAsync(a.b->ptr, 0, a.bytes, h->stream) != hipSuccess) { h->err = "hipMemset failed"; return bail(TFG_ERR_HIP); }
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "sync failed"; return bail(TFG_ERR_HIP); }
  h->plane_state.assign((size_t)n_frames * kNumForc, kOk);  // zero-filled: finite
  *out = h;
  return TFG_OK;
}

int tfg_destroy(tfg_handle* h) {
  if (!h) return TFG_OK;
  (void)hipSetDevice(h->device);
  // work queued on a caller's stream (tfg_set_stream) may still use the buffers
  if (h->stream && h->stream != h->own_stream) (void)hipStreamSynchronize(h->stream);
  if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
  if (h->side) (void)hipStreamSynchronize(h->side);
  delete h;  // the members release what they own
  return TFG_OK;
}

int tfg_set_stream(tfg_handle* h, void* stream) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  h->stream = stream ? static_cast<hipStream_t>(stream) : h->own_stream.v;
  return TFG_OK;
}

int tfg_shared_stream(int device, void** stream) {
  // One non-blocking stream per device for the whole process, created on first
  // use and never destroyed (handles that use it outlive no process).
  static std::mutex mu;
  static hipStream_t streams[64] = {};
  if (!stream) return fail(nullptr, TFG_ERR_ARG, "null stream");
  int count = 0;
  HIPCHK(nullptr, hipGetDeviceCount(&count));
  if (device < 0 || device >= count || device >= 64) return fail(nullptr, TFG_ERR_ARG, "device out of range");
  std::lock_guard<std::mutex> lock(mu);
  if (!streams[device]) {
    int prev = 0;
    HIPCHK(nullptr, hipGetDevice(&prev));
    HIPCHK(nullptr, hipSetDevice(device));
    const hipError_t e = hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
      streams[device] = nullptr;
      return fail(nullptr, TFG_ERR_HIP, "shared stream create failed");
    }
  }
  *stream = streams[device];
  return TFG_OK;
}

int tfg_get_stream(tfg_handle* h, void** stream) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !stream) return fail(h, TFG_ERR_ARG, "null argument");
  *stream = h->stream;
  return TFG_OK;
}

int tfg_set_fuse(tfg_handle* h, int k) {
  if (!h || k < 1) return fail(h, TFG_ERR_ARG, "fuse must be >= 1");
  h->fuse = k;
  return TFG_OK;
}

int tfg_set_step_form(tfg_handle* h, int form) {
  if (!h || (form != TFG_FORM_AUTO && form != TFG_FORM_NAN_SAFE)) return fail(h, TFG_ERR_ARG, "form must be TFG_FORM_AUTO or TFG_FORM_NAN_SAFE");
  h->force_ns = form == TFG_FORM_NAN_SAFE;
  return TFG_OK;
}

int tfg_set_flux(tfg_handle* h, int flux) {
  if (!h || (flux != TFG_FLUX_F32 && flux != TFG_FLUX_F64)) return fail(h, TFG_ERR_ARG, "flux must be TFG_FLUX_F32 or TFG_FLUX_F64");
  h->flux_f64 = flux == TFG_FLUX_F64;  // the fp64 engine computes every flux in fp64 either way
  return TFG_OK;
}

int tfg_set_split(tfg_handle* h, int mode) {
  if (!h || (mode != TFG_SPLIT_AUTO && mode != TFG_SPLIT_OFF && mode != TFG_SPLIT_ON))
    return fail(h, TFG_ERR_ARG, "split must be TFG_SPLIT_AUTO, TFG_SPLIT_OFF or TFG_SPLIT_ON");
  if (int rc = api_sync(h)) return rc;
  h->split_mode = mode;
  return TFG_OK;
}

int tfg_join(tfg_handle* h) {
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  return join_side(h);
}

int tfg_get_split(tfg_handle* h, int* split) {
  if (!h || !split) return fail(h, TFG_ERR_ARG, "null argument");
  *split = split_active(h) ? 1 : 0;
  return TFG_OK;
}

int tfg_set_field(tfg_handle* h, int field, int index, const void* src, int src_dtype, int64_t n,
                  int src_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!src) return fail(h, TFG_ERR_ARG, "null src");
  if (n != h->n) return fail(h, TFG_ERR_ARG, "n = " + std::to_string(n) + " != ny*nx = " + std::to_string(h->n));
  HIPCHK(h, hipSetDevice(h->device));
  // setting a depth writes the previous-step depth the next step reads, so TFG_PREV_DEPTH is slot 0
  if ((field == TFG_OUT_H_SNOW || field == TFG_OUT_H_ICE) && index == TFG_PREV_DEPTH) index = 0;  // same as a plain depth set
  if (is_frame_field(field) && (index < 0 || index >= h->n_frames)) return fail(h, TFG_ERR_ARG, "frame index out of range");
  if (is_hist_field(field) && (index < 0 || index >= h->hist_depth)) return fail(h, TFG_ERR_ARG, "history slot out of range");
  if (field == TFG_ST_CATCH_ID) {
    if (src_dtype != TFG_I32) return fail(h, TFG_ERR_ARG, "catchment ids must be TFG_I32");
    // the ids index the kernels' LDS bins: they are validated before anything
    // reaches h->catch_id (a host source in place, a device source from a
    // staged host copy), so a rejected map leaves the handle as it was
    std::vector<int32_t> tmp;
    const int32_t* hs = static_cast<const int32_t*>(src);
    if (src_on_device) {
      tmp.resize(n);
      HIPCHK(h, hipMemcpyAsync(tmp.data(), src, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      hs = tmp.data();
    }
    for (int64_t i = 0; i < n; ++i)
      if (hs[i] < 0 || hs[i] >= h->n_catch) return fail(h, TFG_ERR_ARG, "catchment id out of [0, n_catch)");
    if (int rc = reserve_zeroed(h, h->catch_id, (size_t)h->n_pad * 4)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->catch_id, src, (size_t)n * 4, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return TFG_OK;
  }
  if (src_dtype != TFG_F32 && src_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "src dtype must be TFG_F32/TFG_F64");
  if (field == TFG_ST_QC) {  // a caller-supplied conduction flux: on until tfg_conduction_off
    if (int rc = ensure_qc(h)) return rc;
    if (int rc = upload(h, h->qc, h->engine, src, src_dtype, n, src_on_device)) return rc;
    h->qc_on = true;
    return note_written(h, h->qc, h->engine, n, src_on_device, &h->qc_state);
  }
  if (field == TFG_ST_WINDOW) {
    if (index < 0 || index >= h->ring_len) return fail(h, TFG_ERR_ARG, "window slot out of range");
    HIPCHK(h, h->wtmp.reserve((size_t)h->n_pad * 8));
    int rc = upload(h, h->wtmp, TFG_F64, src, src_dtype, n, src_on_device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_window_set, grid_for(n), 256, 0, h->stream, h->ring + (int64_t)index * h->n_pad, h->wtmp, n,
                       h->dp.qscale);
    HIPCHK(h, hipGetLastError());
    h->tot_dirty = true;
    // a NaN slot makes the window dirty; a device source is checked lazily (check_state reads the rebuilt totals)
    return note_written(h, h->wtmp, TFG_F64, n, src_on_device, &h->state_state, true);
  }
  int fdt = 0;
  void* dst = field_ptr(h, field, index, &fdt);
  if (!dst) return fail(h, TFG_ERR_ARG, "unknown field id " + std::to_string(field));
  const bool depth = field == TFG_OUT_H_SNOW || field == TFG_OUT_H_ICE || field == TFG_OUT_H_SWE || field == TFG_OUT_H_IWE;
  if (depth && h->depths_derived) {
    // keep the previous-step depths the next update() must see (:895-911)
    hipLaunchKernelGGL(k_materialise_depths, grid_for(h->n_pad), 256, 0, h->stream, h->st, h->n_pad, h->dp.ws, h->dp.wi);
    HIPCHK(h, hipGetLastError());
    h->depths_derived = false;
  }
  if (field == TFG_OUT_H_SNOW || field == TFG_OUT_H_ICE) {
    // user-set depth: both the fp64 state and the visible output
    double* sd = h->st + (field == TFG_OUT_H_SNOW ? S_HSNOW : S_HICE) * h->n_pad;
    int rc = upload(h, sd, TFG_F64, src, src_dtype, n, src_on_device);
    if (rc) return rc;
    if (int rc2 = note_written(h, sd, TFG_F64, n, src_on_device, &h->state_state, true)) return rc2;
    return upload(h, dst, fdt, src, src_dtype, n, src_on_device);
  }
  int rc = upload(h, dst, fdt, src, src_dtype, n, src_on_device);
  if (rc) return rc;
  // finite-data status of what was written (note_written)
  const bool state_field = field == TFG_OUT_H_SWE || field == TFG_OUT_H_IWE || field == TFG_ST_ECCS ||
                           field == TFG_ST_ECCI || field == TFG_ST_ALBEDO || field == TFG_ST_NDAYS;
  uint8_t* status = nullptr;
  if (is_frame_field(field)) {
    const int plane = field == TFG_IN_P ? F_P : field == TFG_IN_T_AIR ? F_T : field == TFG_IN_HUM_SP ? F_Q
                    : field == TFG_IN_P_AIR ? F_PA : F_UZ;
    status = &h->plane_state[(size_t)index * kNumForc + plane];
  } else if (field == TFG_ST_ELEV) {
    status = &h->elev_state;
  } else if (state_field) {
    status = &h->state_state;
  }
  if (status)
    if (int rc2 = note_written(h, dst, fdt, n, src_on_device, status, state_field)) return rc2;
  if (field == TFG_ST_ELEV || field == TFG_ST_SLOPE || field == TFG_ST_ASPECT) h->geo_dirty = true;
  if (field == TFG_ST_SLOPE) {
    if (int rc2 = read_flag(h, &h->slope_invalid, [&] {
          by_type(h->engine, [&](auto t) {
            using R = typename decltype(t)::type;
            hipLaunchKernelGGL((k_check_slope<R>), grid_for(n), 256, 0, h->stream, (const R*)dst, n, h->d_flag);
          });
        }))
      return rc2;
    if (h->slope_invalid) return fail(h, TFG_ERR_DOMAIN, "ERROR: some slope angles are out of range (beta not in [0, pi/2]; bmi_topoflow_glacier.py:1106-1111)");
  }
  return TFG_OK;
}

int tfg_get_field(tfg_handle* h, int field, int index, void* dst, int dst_dtype, int64_t n, int dst_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!dst) return fail(h, TFG_ERR_ARG, "null dst");
  if (n <= 0 || n > h->n) return fail(h, TFG_ERR_ARG, "n outside 1..ny*nx");  // n < ny*nx: the first n cells
  HIPCHK(h, hipSetDevice(h->device));
  if ((field == TFG_OUT_H_SNOW || field == TFG_OUT_H_ICE) && index == TFG_PREV_DEPTH) {
    // the fp64 previous-step depth the next step reads (checkpoint / restart)
    if (dst_dtype != TFG_F32 && dst_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "dst dtype must be TFG_F32/TFG_F64");
    if (h->depths_derived) {
      hipLaunchKernelGGL(k_materialise_depths, grid_for(h->n_pad), 256, 0, h->stream, h->st, h->n_pad, h->dp.ws, h->dp.wi);
      HIPCHK(h, hipGetLastError());
    }
    return download(h, dst, dst_dtype, h->st + (field == TFG_OUT_H_SNOW ? S_HSNOW : S_HICE) * h->n_pad, TFG_F64, n,
                    dst_on_device);
  }
  if (is_frame_field(field) && (index < 0 || index >= h->n_frames)) return fail(h, TFG_ERR_ARG, "frame index out of range");
  if (is_hist_field(field) && (index < 0 || index >= h->hist_depth)) return fail(h, TFG_ERR_ARG, "history slot out of range");
  if (field == TFG_ST_CATCH_ID) {
    if (dst_dtype != TFG_I32) return fail(h, TFG_ERR_ARG, "catchment ids are TFG_I32");
    if (!h->catch_id) return fail(h, TFG_ERR_STATE, "no catchment-id raster set");
    HIPCHK(h, hipMemcpyAsync(dst, h->catch_id, (size_t)n * 4, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return TFG_OK;
  }
  if (dst_dtype != TFG_F32 && dst_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "dst dtype must be TFG_F32/TFG_F64");
  if (field == TFG_ST_QC) {  // zero until a conduction pass or a set (the reference's Qc = 0, :312)
    if (int rc = ensure_qc(h)) return rc;
    return download(h, dst, dst_dtype, h->qc, h->engine, n, dst_on_device);
  }
  if (field == TFG_ST_WINDOW) {
    if (index < 0 || index >= h->ring_len) return fail(h, TFG_ERR_ARG, "window slot out of range");
    HIPCHK(h, h->wtmp.reserve((size_t)h->n_pad * 8));
    hipLaunchKernelGGL(k_window_get, grid_for(n), 256, 0, h->stream, h->wtmp, h->ring + (int64_t)index * h->n_pad, n,
                       1.0 / h->dp.qscale);
    HIPCHK(h, hipGetLastError());
    return download(h, dst, dst_dtype, h->wtmp, TFG_F64, n, dst_on_device);
  }
  int fdt = 0;
  const void* src = field_ptr(h, field, index, &fdt);
  if (!src) return fail(h, TFG_ERR_ARG, "unknown field id " + std::to_string(field));
  if ((field == TFG_OUT_H_SNOW || field == TFG_OUT_H_ICE) && !h->depths_derived) {
    // before any step (or right after a host set) the depths live in the fp64 state
    src = h->st + (field == TFG_OUT_H_SNOW ? S_HSNOW : S_HICE) * h->n_pad;
    fdt = TFG_F64;
  }
  return download(h, dst, dst_dtype, src, fdt, n, dst_on_device);
}

int tfg_init_state(tfg_handle* h) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  HIPCHK(h, hipSetDevice(h->device));
  const DevParams& p = h->dp;
  // Eccs = max((rho_snow*Cp_snow)*h_snow*del_T, 0); del_T = T0 - T_surf(=0)  (:389-395)
  const double del_T = p.T0 - 0.0;
  hipLaunchKernelGGL(k_init_state, grid_for(h->n_pad), 256, 0, h->stream, h->st, h->n_pad, p.rho_snow_Cp_snow, del_T, p.Ecci0,
                     h->engine == TFG_F32 ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(h->tot, 0, (size_t)h->n_pad * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(h->ring, 0, (size_t)h->ring_len * h->n_pad * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(h->hist, 0, (size_t)h->hist_depth * kNumHist * h->n_pad * h->rsz, h->stream));
  HIPCHK(h, hipMemsetAsync(h->slab, 0, (size_t)h->max_blocks * h->n_catch * 6 * 8, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->depths_derived = false;
  h->tot_dirty = false;
  h->initialised = true;
  return TFG_OK;
}

namespace {

int check_step(tfg_handle* h, const tfg_uniforms* u, int64_t nsteps) {
  if (!u) return fail(h, TFG_ERR_ARG, "null uniforms");
  if (!h->initialised) return fail(h, TFG_ERR_STATE, "tfg_init_state() has not been called");
  if (h->slope_invalid) return fail(h, TFG_ERR_DOMAIN, "slope raster invalid (bmi_topoflow_glacier.py:1106-1111)");
  for (int64_t k = 0; k < nsteps; ++k) {
    if (u[k].frame < 0 || u[k].frame >= h->n_frames) return fail(h, TFG_ERR_ARG, "uniforms: frame out of range");
    if (u[k].hist < 0 || u[k].hist >= h->hist_depth) return fail(h, TFG_ERR_ARG, "uniforms: hist slot out of range");
    if (u[k].slot < 0 || u[k].slot >= h->ring_len) return fail(h, TFG_ERR_ARG, "uniforms: ring slot out of range");
  }
  return TFG_OK;
}

// The launches of nsteps steps whose uniforms the device reads at d_u (u is
// the host copy of the same records).
int64_t chunks_of(int64_t cells) { return (cells / kCellsPerThread + kBlock - 1) / kBlock; }
int fused_blocks(const tfg_handle* h) {  // k_fused steps the whole plane stride
  return (int)std::min<int64_t>(std::max<int64_t>(chunks_of(h->n_pad), 1), h->max_blocks);
}

// Work a launch of the step kernels depends on: window totals after slots were
// set, and the per-cell geometry after the static rasters changed.
int prepare_steps(tfg_handle* h) {
  if (h->tot_dirty || h->geo_dirty)  // rewrites planes a split launch's second part may still read
    if (int rc = api_sync(h)) return rc;
  if (h->tot_dirty) {  // window slots were set: rebuild the running totals
    hipLaunchKernelGGL(k_window_total, grid_for(h->n_pad), 256, 0, h->stream, h->tot, h->ring, h->ring_len, h->n_pad);
    HIPCHK(h, hipGetLastError());
    h->tot_dirty = false;
  }
  if (h->geo_dirty) {
    by_type(h->engine, [&](auto t) {  // the fast engine's solar geometry, the exact engine's CellStatic planes
      using R = typename decltype(t)::type;
      if constexpr (std::is_same_v<R, float>)
        hipLaunchKernelGGL((k_prepare_geo<R>), grid_for(h->n_pad), 256, 0, h->stream, h->dp, (const R*)h->stat.ptr, h->geo, h->n_pad);
      else
        hipLaunchKernelGGL((k_prepare_static<R>), grid_for(h->n_pad), 256, 0, h->stream, h->dp, (const R*)h->stat.ptr,
                           (double*)h->geo.ptr, h->n_pad);
    });
    HIPCHK(h, hipGetLastError());
    h->geo_dirty = false;
  }
  return TFG_OK;
}

// Launches of at least this many steps check unknown data before choosing the
// fp32 step form (a synchronous device check); shorter ones run NaN-safe.
constexpr int kVerifySteps = 8;

// The state's finite-data status: the fp64 state planes and the window totals
// (after prepare_steps has rebuilt them).  Synchronous.
int check_state(tfg_handle* h) {
  const int64_t np = h->n_pad;
  const int gb = grid_for(h->n);
  bool bad = false;
  // the state planes, the albedo plane in the engine's type (fp32 for the fp32 engine)
  int rc = read_flag(h, &bad, [&] {
    hipLaunchKernelGGL((k_nonfinite<double>), gb, 256, 0, h->stream, (const double*)h->st, h->n, np, S_ALB, h->d_flag);
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      hipLaunchKernelGGL((k_nonfinite<R>), gb, 256, 0, h->stream, (const R*)(h->st + S_ALB * np), h->n, (int64_t)0, 1, h->d_flag);
    });
    hipLaunchKernelGGL((k_nonfinite<double>), gb, 256, 0, h->stream, (const double*)(h->st + (S_ALB + 1) * np), h->n, np,
                       kNumState - S_ALB - 1, h->d_flag);
  });
  if (rc == TFG_OK && !bad)
    rc = read_flag(h, &bad, [&] { hipLaunchKernelGGL(k_window_nan, gb, 256, 0, h->stream, h->tot, h->n, h->d_flag); });
  if (rc == TFG_OK) h->state_state = bad ? kDirty : kOk;
  return rc;
}

// The fp32 engine's step form for one launch of K steps (tfg_physics.hpp,
// "Missing data"): the clean form when the launch's forcing frames (or the
// tfg_update inputs), the elevation raster, the Qc plane in use, the state and
// the window are known to hold only finite values; the NaN-safe form
// otherwise.  Unknown data is checked first when the launch is long enough to
// pay for a synchronous check.
int choose_form(tfg_handle* h, const tfg_uniforms* u, int K, const IoArgs& io, bool* ns) {
  const bool check = K >= kVerifySteps;
  bool inputs_ok = true;
  if (io.in) {
    inputs_ok = io.in_state == kOk;
  } else {
    if (check) {
      // every frame the launch reads that holds a plane of unknown status is
      // checked on the device, all of them before one host wait
      int nf = 0;
      for (int k = 0; k < K; ++k) {
        const int fr = u[k].frame;
        const uint8_t* ps = &h->plane_state[(size_t)fr * kNumForc];
        if (std::find(ps, ps + kNumForc, kUnknown) == ps + kNumForc) continue;
        if (std::find(h->chk_frames.begin(), h->chk_frames.begin() + nf, fr) != h->chk_frames.begin() + nf) continue;
        if ((int)h->chk_frames.size() <= nf) h->chk_frames.resize(nf + 1);
        h->chk_frames[nf++] = fr;
      }
      if (nf) {
        HIPCHK(h, hipMemsetAsync(h->d_flag, 0, (size_t)nf * kNumForc * 4, h->stream));
        const dim3 grid(std::max(1, std::min(grid_for(h->n), 2048)), kNumForc);
        for (int j = 0; j < nf; ++j) {
          const char* fp = h->forc.bytes() + (size_t)h->chk_frames[j] * kNumForc * h->n_pad * h->rsz;
          hipLaunchKernelGGL((k_nonfinite_planes<float>), grid, 256, 0, h->stream, (const float*)fp, h->n, h->n_pad,
                             h->d_flag + j * kNumForc);
        }
        HIPCHK(h, hipGetLastError());
        std::vector<int32_t> flags((size_t)nf * kNumForc);
        HIPCHK(h, hipMemcpyAsync(flags.data(), h->d_flag, flags.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int j = 0; j < nf; ++j) {
          uint8_t* ps = &h->plane_state[(size_t)h->chk_frames[j] * kNumForc];
          for (int f = 0; f < kNumForc; ++f)
            if (ps[f] == kUnknown) ps[f] = flags[(size_t)j * kNumForc + f] ? kDirty : kOk;
        }
      }
    }
    for (int k = 0; k < K; ++k) {
      const uint8_t* ps = &h->plane_state[(size_t)u[k].frame * kNumForc];
      for (int f = 0; f < kNumForc; ++f) inputs_ok &= ps[f] == kOk;
    }
  }
  if (check && (h->state_state == kUnknown || (h->state_state == kDirty && --h->state_recheck <= 0))) {
    if (int rc = api_sync(h)) return rc;  // the state a split launch's second part writes
    if (int rc = check_state(h)) return rc;
    if (h->state_state == kDirty) h->state_recheck = kVerifySteps;  // launches until the next look
  }
  if (h->qc_on && h->qc_state == kUnknown && check)
    if (int rc = check_finite(h, h->qc, h->engine, h->n, &h->qc_state)) return rc;
  if (h->elev_state == kUnknown && check)  // a device-sourced elevation raster (tfg_set_field)
    if (int rc = check_finite(h, h->stat, h->engine, h->n, &h->elev_state)) return rc;
  *ns = h->force_ns ||
        !(inputs_ok && h->state_state == kOk && h->elev_state == kOk && (!h->qc_on || h->qc_state == kOk));
  return TFG_OK;
}

// After a launch of the fp32 engine: the NaN-safe form may have carried missing data into the state.
void note_form(tfg_handle* h, bool ns) {
  if (!ns) return;
  ++h->ns_launches;
  if (h->state_state == kOk) h->state_state = kUnknown;
}

// The step table of u[0 .. nsteps) (tfg_fused.hpp, StepAddr): byte offsets in
// the handle's engine type and plane stride.  check_step has held every index
// to its buffer.  tfg_update's step (io) reads its forcing at the host block
// itself: a zero offset.
void step_table(const tfg_handle* h, const tfg_uniforms* u, int64_t nsteps, StepAddr* t, bool io = false) {
  const int64_t plane = h->n_pad * (int64_t)h->rsz;
  for (int64_t k = 0; k < nsteps; ++k)
    t[k] = {io ? 0 : u[k].frame * kNumForc * plane, u[k].slot * h->n_pad * (int64_t)sizeof(int32_t),
            u[k].hist * kNumHist * plane, 0};
}
// Bytes of nsteps staged steps: the uniforms, then their table.  A launch of K
// steps from k0 reads records k0 .. k0 + K - 1 only (k_fused clamps its
// read-ahead to the launch's last record, it does not repeat trailing records),
// and k0 + K <= nsteps: no read passes the table's end.
constexpr size_t stage_bytes(int64_t nsteps) { return (size_t)nsteps * (sizeof(tfg_uniforms) + sizeof(StepAddr)); }
static_assert(sizeof(tfg_uniforms) % alignof(StepAddr) == 0 && sizeof(tfg_uniforms) % 32 == 0,
              "the table after the uniforms keeps its records aligned");
const StepAddr* table_of(const tfg_uniforms* d_u, int64_t nsteps) { return reinterpret_cast<const StepAddr*>(d_u + nsteps); }

// d_t (the side stream's copy: d_t2) is the step table of the records at d_u.
int launch_steps(tfg_handle* h, const tfg_uniforms* d_u, const StepAddr* d_t, const StepAddr* d_t2, const tfg_uniforms* u,
                 int64_t nsteps, const IoArgs& io = IoArgs(), bool split = false) {
  if (int rc = prepare_steps(h)) return rc;
  const int blocks = fused_blocks(h);
  const size_t lds = (size_t)kWaves * h->n_catch * 6 * sizeof(double);
  // a fused launch reads each step's expiring window slot 1 (fp64 engine) or
  // kPrefetchFast (fp32 engine) steps ahead: a shorter window runs unfused
  // (see the prefetch note in k_fused)
  const int fuse = h->ring_len > (h->engine == TFG_F32 ? kPrefetchFast : 1) ? h->fuse : 1;
  const bool one_cell = h->engine == TFG_F64 && h->n == 1 && !io.in;  // k_cell_run
  for (int64_t k0 = 0; k0 < nsteps; k0 += fuse) {
    const int K = (int)std::min<int64_t>(fuse, nsteps - k0);
    int rc = TFG_OK;
    if (one_cell) {
      hipLaunchKernelGGL(k_cell_run, 1, 64 * tfg::kCellWaves, 0, h->stream, step_args(h, K, io), d_u + k0,
                         (const double*)h->geo.ptr, h->catch_id, h->st, h->tot, h->ring, (const double*)h->forc.ptr,
                         (double*)h->hist.ptr, h->slab, h->qc_on ? (const double*)h->qc.ptr : nullptr,
                         h->depths_derived ? 0 : 1);
      HIPCHK(h, hipGetLastError());
    } else if (h->engine == TFG_F32 && split && !io.in) {
      // two parts on two streams: the first on the handle's stream, the second
      // on the side stream with its own uniforms (tfg_step copied them there)
      bool ns = true;
      if ((rc = choose_form(h, u + k0, K, io, &ns))) return rc;
      if ((rc = fork_side(h))) return rc;
      // an odd chunk count for the first part: the parts' planes then do not sit a
      // power of two apart (+0.3-0.5 % at 2048^2 against an even split, same box)
      const int64_t chA = (chunks_of(h->n_pad) / 2) | 1, chB = chunks_of(h->n_pad) - chA;
      const int64_t nA = chA * kBlock * kCellsPerThread;
      const bool fit = chA + chB <= h->max_blocks;  // one workgroup per chunk, as unsplit
      const int bA = (int)(fit ? chA : std::min<int64_t>(chA, h->max_blocks / 2));
      const int bB = (int)(fit ? chB : std::min<int64_t>(chB, h->max_blocks / 2));
      const Part pa = {0, nA, std::min(h->n, nA), 0, h->stream};
      const Part pb = {nA, h->n_pad - nA, std::max<int64_t>(h->n - nA, 0), bA, h->side};
      if ((rc = launch_fused<float, false>(h, d_u + k0, d_t + k0, K, bA, lds, io, ns, &pa))) return rc;
      if ((rc = launch_fused<float, false>(h, h->d_u2 + k0, d_t2 + k0, K, bB, lds, io, ns, &pb))) return rc;
      h->side_busy = true;
      note_form(h, ns);
    } else if (h->engine == TFG_F32) {
      bool ns = true;
      if ((rc = choose_form(h, u + k0, K, io, &ns))) return rc;
      rc = launch_fused<float, false>(h, d_u + k0, d_t + k0, K, blocks, lds, io, ns);
      note_form(h, ns);
    } else {
      rc = launch_fused<double, true>(h, d_u + k0, d_t + k0, K, blocks, lds, io, false);
    }
    if (rc) return rc;
    h->depths_derived = true;
  }
  h->last_hist = u[nsteps - 1].hist;
  return TFG_OK;
}

}  // namespace

int tfg_step(tfg_handle* h, const tfg_uniforms* u, int64_t nsteps) {
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (nsteps <= 0) return TFG_OK;
  if (int rc = check_step(h, u, nsteps)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const bool split = split_active(h);
  if (split) {
    if (int rc = ensure_side(h)) return rc;
  } else if (int rc = api_sync(h)) {  // a handle that stopped splitting (tfg_set_split)
    return rc;
  }
  // stage uniforms: pinned double buffer -> device array (and the side stream's copy)
  const size_t bytes = stage_bytes(nsteps);
  StageRing::Slot* s = nullptr;
  HIPCHK(h, h->u_ring.acquire(bytes, false, &s));
  if (h->d_u.cap < bytes) {
    // the previous launches may still read d_u: wait before reallocating
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->d_u.reserve(bytes));
  }
  // the uniforms and, right after them, their step table: one copy
  tfg_uniforms* h_u = static_cast<tfg_uniforms*>(s->host.ptr);
  std::memcpy(h_u, u, (size_t)nsteps * sizeof(tfg_uniforms));
  step_table(h, u, nsteps, reinterpret_cast<StepAddr*>(h_u + nsteps));
  HIPCHK(h, hipMemcpyAsync(h->d_u, h_u, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, StageRing::commit(*s, h->stream));
  if (split) {
    if (h->d_u2.cap < bytes) {
      HIPCHK(h, hipStreamSynchronize(h->side));  // its launches may still read d_u2
      HIPCHK(h, h->d_u2.reserve(bytes));
    }
    HIPCHK(h, s->done2.create());
    HIPCHK(h, hipMemcpyAsync(h->d_u2, h_u, bytes, hipMemcpyHostToDevice, h->side));
    HIPCHK(h, hipEventRecord(s->done2, h->side));
  }
  return launch_steps(h, h->d_u, table_of(h->d_u, nsteps), split ? table_of(h->d_u2, nsteps) : nullptr, u, nsteps, IoArgs(),
                      split);
}

int tfg_get_diag(tfg_handle* h, double* out, int n_catch) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !out) return fail(h, TFG_ERR_ARG, "null argument");
  if (n_catch != h->n_catch) return fail(h, TFG_ERR_ARG, "n_catch mismatch");
  HIPCHK(h, hipSetDevice(h->device));
  const int nb = n_catch * 6;
  hipLaunchKernelGGL(k_diag_reduce, nb, kBlock, 0, h->stream, h->slab, h->max_blocks, nb, h->diag);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, h->diag, (size_t)n_catch * 6 * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // P_max of an empty history is 0 like the reference's initial P_max (:314)
  for (int c = 0; c < n_catch; ++c) if (out[c * 6 + 5] == -INFINITY) out[c * 6 + 5] = 0.0;
  return TFG_OK;
}

int tfg_catchment_series(tfg_handle* h, int field, int hist0, int nslots, double* out, int out_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!out) return fail(h, TFG_ERR_ARG, "null out");
  HistWindow w;
  if (int rc = hist_window(h, "catchment series", field, hist0, nslots, &w)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const int blocks = series_blocks(h->n, h->n_catch);
  const int row_len = kSeriesBatch * h->n_catch;
  // partials [blocks][kSeriesBatch][n_catch]; a host call's result [hist_depth][n_catch]
  HIPCHK(h, reserve_idle(h, h->rd_part_sum, (size_t)blocks * row_len * 8));
  if (!out_on_device) HIPCHK(h, reserve_idle(h, h->rd_out_sum, (size_t)h->hist_depth * h->n_catch * 8));
  double* dout = out_on_device ? out : h->rd_out_sum;
  const size_t lds = (size_t)row_len * 8;
  for (int j0 = 0; j0 < w.nslots; j0 += kSeriesBatch) {
    const auto b = w.batch(j0, kSeriesBatch);
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, blocks, kBlock, lds, h->stream, (const R*)w.plane, w.stride, w.depth, b.slot0, b.nb,
                           h->catch_id, h->n, h->n_catch, h->rd_part_sum);
      };
      if (h->catch_id) launch(k_catch_series<R, true>);
      else launch(k_catch_series<R, false>);
    });
    HIPCHK(h, hipGetLastError());
    const int nent = b.nb * h->n_catch;
    hipLaunchKernelGGL(k_series_reduce, (nent + 15) / 16, kBlock, 0, h->stream, h->rd_part_sum, blocks, row_len, nent,
                       dout + (int64_t)j0 * h->n_catch);
    HIPCHK(h, hipGetLastError());
  }
  if (!out_on_device) {
    HIPCHK(h, hipMemcpyAsync(out, dout, (size_t)nslots * h->n_catch * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return TFG_OK;
}

int tfg_band_series(tfg_handle* h, int field, int hist0, int nslots, const tfg_bands* b, double* sum, int64_t* count,
                    int64_t* cells, int out_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!b || !b->edges) return fail(h, TFG_ERR_ARG, "band series: null bands or edges");
  if (!sum && !count && !cells) return fail(h, TFG_ERR_ARG, "band series: no output requested");
  if (b->n_bands < 1 || b->n_bands > kBandMaxBands) return fail(h, TFG_ERR_ARG, "band series: n_bands outside 1..64");
  if ((int64_t)h->n_catch * b->n_bands > kBandMaxKeys)
    return fail(h, TFG_ERR_ARG, "band series: n_catch * n_bands = " + std::to_string((int64_t)h->n_catch * b->n_bands) + " > 2048");
  BandEdges edges{};
  for (int k = 0; k <= b->n_bands; ++k) {
    edges.e[k] = b->edges[k];
    if (!std::isfinite(edges.e[k])) return fail(h, TFG_ERR_ARG, "band series: edge " + std::to_string(k) + " is not finite");
    if (k && !(edges.e[k] > edges.e[k - 1])) return fail(h, TFG_ERR_ARG, "band series: edges must be strictly ascending");
  }
  if (count && b->threshold != b->threshold) return fail(h, TFG_ERR_ARG, "band series: NaN threshold");
  HistWindow w;
  if (int rc = hist_window(h, "band series", field, hist0, nslots, &w)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const int K = h->n_catch * b->n_bands;
  const bool planes = sum || count;               // without them one cells-only launch, no plane read
  const int NB = planes ? band_batch(K) : 0;
  const int blocks = band_blocks(h->n, K);
  const int row_sum = NB * K, row_int = NB * K + K;
  // partials [blocks][NB][K] sums, [blocks][NB * K + K] counts then cells; a host call's [hist_depth][K] sums, [hist_depth][K] counts then [K] cells
  if (sum) HIPCHK(h, reserve_idle(h, h->rd_part_sum, (size_t)blocks * row_sum * 8));
  HIPCHK(h, reserve_idle(h, h->rd_part_int, (size_t)blocks * (band_batch(K) * K + K) * 4));
  if (!out_on_device) {
    if (sum) HIPCHK(h, reserve_idle(h, h->rd_out_sum, (size_t)h->hist_depth * K * 8));
    HIPCHK(h, reserve_idle(h, h->rd_out_int, ((size_t)h->hist_depth * K + K) * 8));
  }
  double* dsum = out_on_device ? sum : (double*)h->rd_out_sum;
  int64_t* dcount = out_on_device ? count : (int64_t*)h->rd_out_int;
  int64_t* dcells = out_on_device ? cells : (int64_t*)h->rd_out_int + (int64_t)h->hist_depth * K;
  const size_t lds = band_lds_bytes(NB, K);
  const int step = planes ? NB : nslots;  // the cells-only call: one trip
  for (int j0 = 0; j0 < nslots; j0 += step) {
    const int nb = planes ? w.batch(j0, step).nb : 1, slot0 = w.batch(j0, step).slot0;
    const int what = (sum ? kBandSum : 0) | (count ? kBandCount : 0) | (cells && j0 == 0 ? kBandCells : 0);
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, blocks, kBlock, lds, h->stream, (const R*)w.plane, w.stride, w.depth, slot0, nb,
                           h->catch_id, (const R*)h->stat.bytes(), edges, b->n_bands, b->threshold, what, h->n, K,
                           h->rd_part_sum, h->rd_part_int);
      };
      auto with_nb = [&](auto c) {
        constexpr bool C = decltype(c)::value;
        switch (NB) {
          case 8: launch(k_band_series<R, C, 8>); break;
          case 4: launch(k_band_series<R, C, 4>); break;
          case 2: launch(k_band_series<R, C, 2>); break;
          default: launch(k_band_series<R, C, 0>); break;
        }
      };
      if (h->catch_id) with_nb(std::true_type{});
      else with_nb(std::false_type{});
    });
    HIPCHK(h, hipGetLastError());
    const int nent = nb * K;
    if (sum) {
      hipLaunchKernelGGL(k_series_reduce, (nent + 15) / 16, kBlock, 0, h->stream, h->rd_part_sum, blocks, row_sum, nent,
                         dsum + (int64_t)j0 * K);
      HIPCHK(h, hipGetLastError());
    }
    if (count) {
      hipLaunchKernelGGL(k_band_reduce_int, (nent + 15) / 16, kBlock, 0, h->stream, h->rd_part_int, blocks, row_int, nent,
                         dcount + (int64_t)j0 * K);
      HIPCHK(h, hipGetLastError());
    }
    if (what & kBandCells) {
      hipLaunchKernelGGL(k_band_reduce_int, (K + 15) / 16, kBlock, 0, h->stream, h->rd_part_int + row_sum, blocks, row_int,
                         K, dcells);
      HIPCHK(h, hipGetLastError());
    }
  }
  if (!out_on_device) {
    if (sum) HIPCHK(h, hipMemcpyAsync(sum, dsum, (size_t)nslots * K * 8, hipMemcpyDeviceToHost, h->stream));
    if (count) HIPCHK(h, hipMemcpyAsync(count, dcount, (size_t)nslots * K * 8, hipMemcpyDeviceToHost, h->stream));
    if (cells) HIPCHK(h, hipMemcpyAsync(cells, dcells, (size_t)K * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return TFG_OK;
}

extern "C++" {  // a template below
namespace {

// The tables of grid g on the device (coarse_plan): kept while the calls pass the same grid.
int coarse_prepare(tfg_handle* h, const tfg_forcing_grid& g) {
  tfg_forcing_grid key = g;
  key.method = 0;  // not read: the key rule is the nearest node's
  key.pad = 0;
  if (h->coarse_valid && !std::memcmp(&key, &h->coarse_grid, sizeof key)) return TFG_OK;
  h->coarse_valid = false;
  std::vector<int32_t> tab;
  const CoarsePlan p = coarse_plan(h->ny, h->nx, key, 16 / (int)h->rsz, tab);
  if ((int64_t)p.nseg * p.ntiles > INT32_MAX) return fail(h, TFG_ERR_ARG, "coarse series: too many row segments x column tiles");
  const size_t bytes = tab.size() * sizeof(int32_t);
  StageRing::Slot* s = nullptr;  // through the pinned ring: one queued copy, no host wait
  HIPCHK(h, h->in_ring.acquire(bytes, false, &s));
  std::memcpy(s->host.ptr, tab.data(), bytes);
  HIPCHK(h, reserve_idle(h, h->coarse_tab, bytes));
  HIPCHK(h, hipMemcpyAsync(h->coarse_tab.ptr, s->host.ptr, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, StageRing::commit(*s, h->stream));
  h->coarse = p;
  h->coarse_grid = key;
  h->coarse_valid = true;
  return TFG_OK;
}

// out[nb][gny][gnx] from a batch's partials, by the plan's threads per entry.
template <class T, class O>
int coarse_fold(tfg_handle* h, const T* part, int nb, const tfg_forcing_grid& g, O* out) {
  const CoarsePlan& p = h->coarse;
  const int32_t* tab = h->coarse_tab;
  const int64_t nent = (int64_t)nb * g.gny * g.gnx, per = kBlock / p.fold_th, blocks = (nent + per - 1) / per;
  if (blocks > INT32_MAX) return fail(h, TFG_ERR_ARG, "coarse series: too many nodes for this geometry's fold");
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, (int)blocks, kBlock, 0, h->stream, part, nb, g.gny, g.gnx, p.P, tab + p.o_segj, tab + p.o_pairi, out);
  };
  switch (p.fold_th) {
    case 1: launch(k_coarse_fold<T, O, 1>); break;
    case 16: launch(k_coarse_fold<T, O, 16>); break;
    default: launch(k_coarse_fold<T, O, 256>); break;
  }
  HIPCHK(h, hipGetLastError());
  return TFG_OK;
}

}  // namespace
}  // extern "C++"

int tfg_coarse_series(tfg_handle* h, int field, int hist0, int nslots, const tfg_forcing_grid* g, double threshold,
                      double* sum, int64_t* count, int64_t* cells, int out_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!g) return fail(h, TFG_ERR_ARG, "coarse series: null grid");
  if (!sum && !count && !cells) return fail(h, TFG_ERR_ARG, "coarse series: no output requested");
  if (g->gny < 1 || g->gnx < 1) return fail(h, TFG_ERR_ARG, "coarse series: gny and gnx must be >= 1");
  if ((int64_t)g->gny * g->gnx >= ((int64_t)1 << 29))  // tfg_set_gridded_forcing's limit
    return fail(h, TFG_ERR_ARG, "coarse series: gny * gnx must stay under 2^29");
  if (!std::isfinite(g->y0) || !std::isfinite(g->x0) || !std::isfinite(g->sy) || !std::isfinite(g->sx))
    return fail(h, TFG_ERR_ARG, "coarse series: y0, x0, sy and sx must be finite");
  if (g->row0 < 0) return fail(h, TFG_ERR_ARG, "coarse series: row0 must be >= 0");
  if (count && threshold != threshold) return fail(h, TFG_ERR_ARG, "coarse series: NaN threshold");
  HistWindow w;  // checked for a cells-only call too
  if (int rc = hist_window(h, "coarse series", field, hist0, nslots, &w)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = coarse_prepare(h, *g)) return rc;
  const CoarsePlan& p = h->coarse;
  const int32_t* tab = h->coarse_tab;
  const size_t nodes = (size_t)g->gny * (size_t)g->gnx;
  const size_t part_len = (size_t)p.nseg * kCoarseBatch * p.P;
  // partials [nseg][kCoarseBatch][P] sums and counts; a host call's copy of one batch, [kCoarseBatch][nodes] each, then [nodes] cells
  if (sum) HIPCHK(h, reserve_idle(h, h->rd_part_sum, part_len * 8));
  if (count) HIPCHK(h, reserve_idle(h, h->rd_part_int, part_len * 4));
  if (!out_on_device) {
    if (sum) HIPCHK(h, reserve_idle(h, h->rd_out_sum, kCoarseBatch * nodes * 8));
    HIPCHK(h, reserve_idle(h, h->rd_out_int, (kCoarseBatch * nodes + nodes) * 8));
  }
  if (cells) {  // rows(J) cols(I): no plane is read
    int64_t* dcells = out_on_device ? cells : (int64_t*)h->rd_out_int + kCoarseBatch * nodes;
    hipLaunchKernelGGL(k_coarse_cells, (int)std::min<size_t>((nodes + kBlock - 1) / kBlock, 4096), kBlock, 0, h->stream,
                       tab + p.o_rows, tab + p.o_cols, g->gny, g->gnx, dcells);
    HIPCHK(h, hipGetLastError());
    if (!out_on_device) HIPCHK(h, hipMemcpyAsync(cells, dcells, nodes * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (sum || count) {
    const int v = 16 / (int)h->rsz;
    const bool vec = h->nx % v == 0 && (uintptr_t)w.plane % 16 == 0 && (w.stride * (int64_t)h->rsz) % 16 == 0;
    for (int j0 = 0; j0 < w.nslots; j0 += kCoarseBatch) {
      const auto b = w.batch(j0, kCoarseBatch);
      const int nb = b.nb;
      by_type(h->engine, [&](auto t) {
        using R = typename decltype(t)::type;
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(kern, p.nseg * p.ntiles, kBlock, 0, h->stream, (const R*)w.plane, w.stride, w.depth, b.slot0, nb,
                             (int)h->nx, tab + p.o_seg, tab + p.o_pcol, p.ntiles, p.P, threshold,
                             (double*)h->rd_part_sum, (int32_t*)h->rd_part_int);
        };
        auto with_what = [&](auto vc) {
          constexpr bool VEC = decltype(vc)::value;
          if (sum && count) launch(k_coarse_series<R, VEC, true, true>);
          else if (sum) launch(k_coarse_series<R, VEC, true, false>);
          else launch(k_coarse_series<R, VEC, false, true>);
        };
        if (vec) with_what(std::true_type{});
        else with_what(std::false_type{});
      });
      HIPCHK(h, hipGetLastError());
      // a device output takes the batch's rows in place; a host output is copied out batch by batch
      if (sum) {
        double* dsum = out_on_device ? sum + (size_t)j0 * nodes : (double*)h->rd_out_sum;
        if (int rc = coarse_fold(h, (const double*)h->rd_part_sum, nb, *g, dsum)) return rc;
        if (!out_on_device)
          HIPCHK(h, hipMemcpyAsync(sum + (size_t)j0 * nodes, dsum, (size_t)nb * nodes * 8, hipMemcpyDeviceToHost, h->stream));
      }
      if (count) {
        int64_t* dcount = out_on_device ? count + (size_t)j0 * nodes : (int64_t*)h->rd_out_int;
        if (int rc = coarse_fold(h, (const int32_t*)h->rd_part_int, nb, *g, dcount)) return rc;
        if (!out_on_device)
          HIPCHK(h, hipMemcpyAsync(count + (size_t)j0 * nodes, dcount, (size_t)nb * nodes * 8, hipMemcpyDeviceToHost, h->stream));
      }
    }
  }
  if (!out_on_device) HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

int tfg_cell_aggregate(tfg_handle* h, int field, int hist0, int nslots, const tfg_cell_stats* acc, int init) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!acc) return fail(h, TFG_ERR_ARG, "cell aggregate: null acc");
  if (!acc->sum && !acc->vmax && !acc->vmin && !acc->count) return fail(h, TFG_ERR_ARG, "cell aggregate: no statistic requested");
  HistWindow w;
  if (int rc = hist_window(h, "cell aggregate", field, hist0, nslots, &w)) return rc;
  if (acc->count && acc->threshold != acc->threshold) return fail(h, TFG_ERR_ARG, "cell aggregate: NaN threshold");
  HIPCHK(h, hipSetDevice(h->device));
  auto aligned = [](const void* p, int bit) { return p && ((uintptr_t)p & 15) == 0 ? bit : 0; };
  const int vec = aligned(acc->sum, kAggVecSum) | aligned(acc->vmax, kAggVecMax) | aligned(acc->vmin, kAggVecMin) |
                  aligned(acc->count, kAggVecCount);
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL(k_cell_aggregate<R>, aggregate_blocks(h->n, 16 / (int)sizeof(R)), kBlock, 0, h->stream,
                       (const R*)w.plane, w.stride, w.depth, hist0, nslots, h->n, acc->sum, (R*)acc->vmax, (R*)acc->vmin,
                       acc->count, acc->threshold, init != 0 ? 1 : 0, vec);
  });
  HIPCHK(h, hipGetLastError());
  return TFG_OK;
}

int tfg_reset_diag(tfg_handle* h) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(h->slab, 0, (size_t)h->max_blocks * h->n_catch * 6 * 8, h->stream));
  return TFG_OK;
}

int tfg_selftest_powers(int device, const double* x, int64_t n, int which, double* out) {
  if (!x || !out || n < 0 || which < 0 || which > 13) return fail(nullptr, TFG_ERR_ARG, "bad arguments");
  if (n == 0) return TFG_OK;
  HIPCHK(nullptr, hipSetDevice(device));
  double* d = nullptr;
  HIPCHK(nullptr, hipMalloc((void**)&d, (size_t)n * 16));
  hipError_t e = hipMemcpy(d, x, (size_t)n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_selftest_powers, grid_for(n), 256, 0, nullptr, d, d + n, n, which);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + n, (size_t)n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(nullptr, TFG_ERR_HIP, std::string("tfg_selftest_powers: ") + hipGetErrorString(e));
  return TFG_OK;
}

#ifdef TFG_WG_TIMING
// diagnostic builds only: the last k_fused<float> launch's per-workgroup
// [start, end, (xcc << 32) | cu] records (tfg_fused.hpp, g_wg_times)
int tfg_debug_wg_times(unsigned long long* out, int n) {
  if (!out || n < 0 || n > TFG_WG_TIMING) return fail(nullptr, TFG_ERR_ARG, "bad arguments");
  HIPCHK(nullptr, hipDeviceSynchronize());
  HIPCHK(nullptr, hipMemcpyFromSymbol(out, HIP_SYMBOL(tfg_kern::g_wg_times), (size_t)n * 24));
  return TFG_OK;
}
#endif

int tfg_nan_safe_launches(tfg_handle* h, int64_t* count) {
  if (!h || !count) return fail(h, TFG_ERR_ARG, "null argument");
  *count = h->ns_launches;
  return TFG_OK;
}

int tfg_sync(tfg_handle* h) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

int tfg_fill_synthetic(tfg_handle* h, uint64_t seed, int64_t row0, int64_t nx_global, const float* diurnal,
                       int n_frames) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !diurnal) return fail(h, TFG_ERR_ARG, "null argument");
  if (n_frames != h->n_frames) return fail(h, TFG_ERR_ARG, "n_frames mismatch");
  if (nx_global != h->nx) return fail(h, TFG_ERR_ARG, "row-block shards must span full rows (nx_global == nx)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_diurnal.reserve((size_t)n_frames * 4));
  HIPCHK(h, hipMemcpyAsync(h->d_diurnal, diurnal, (size_t)n_frames * 4, hipMemcpyHostToDevice, h->stream));
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL((k_fill_synthetic<R>), grid_for(h->n), 256, 0, h->stream, (R*)h->forc.ptr, (R*)h->stat.ptr, h->st,
                       h->n, h->n_pad, h->nx, row0, nx_global, seed, h->d_diurnal, n_frames);
  });
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->slope_invalid = false;
  h->geo_dirty = true;
  // the generator writes finite forcing, statics and depths
  std::fill(h->plane_state.begin(), h->plane_state.end(), kOk);
  h->elev_state = kOk;
  h->state_state = kOk;
  return tfg_init_state(h);
}

namespace {
int launch_scatter(tfg_handle* h, int frame, const void* dsrc, int src_dtype, int64_t n);
int launch_gather(tfg_handle* h, int hist, void* gdst, int dst_dtype, int64_t n);
}  // namespace

int tfg_set_inputs(tfg_handle* h, int frame, const void* src, int src_dtype, int64_t n, int src_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!src) return fail(h, TFG_ERR_ARG, "null src");
  if (n != h->n) return fail(h, TFG_ERR_ARG, "n != ny*nx");
  if (frame < 0 || frame >= h->n_frames) return fail(h, TFG_ERR_ARG, "frame index out of range");
  if (src_dtype != TFG_F32 && src_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "src dtype must be TFG_F32/TFG_F64");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)5 * n * dtype_size(src_dtype);
  const void* dsrc = src;
  StageRing::Slot* s = nullptr;
  if (!src_on_device) {  // borrowed for this call only: through the staging ring
    HIPCHK(h, h->in_ring.acquire(bytes, true, &s));
    std::memcpy(s->host.ptr, src, bytes);
    HIPCHK(h, hipMemcpyAsync(s->dev.ptr, s->host.ptr, bytes, hipMemcpyHostToDevice, h->stream));
    dsrc = s->dev.ptr;
  }
  if (h->engine == TFG_F32) {  // finite-data tracking: host inputs are checked here, device inputs later
    for (int f = 0; f < 5; ++f) {
      uint8_t st = kUnknown;
      if (!src_on_device)
        st = src_dtype == TFG_F64 ? host_finite_as_f32(static_cast<const double*>(src) + (size_t)f * n, n)
                                  : host_finite_as_f32(static_cast<const float*>(src) + (size_t)f * n, n);
      h->plane_state[(size_t)frame * kNumForc + kBmiToPlane[f]] = st;
    }
  }
  if (int rc = launch_scatter(h, frame, dsrc, src_dtype, n)) return rc;
  if (s) HIPCHK(h, StageRing::commit(*s, h->stream));
  return TFG_OK;
}

namespace {
// The checks of a tfg_downscale (NULL: every term off); *on: whether a term is on.
int check_downscale(tfg_handle* h, const tfg_downscale* ds, const char* what, bool* on) {
  *on = false;
  if (!ds) return TFG_OK;
  const std::string w = std::string(what) + ": ";
  if (!std::isfinite(ds->lapse_T) || !std::isfinite(ds->grad_P)) return fail(h, TFG_ERR_ARG, w + "lapse_T and grad_P must be finite");
  if (!std::isfinite(ds->rh_max) || ds->rh_max < 0.0) return fail(h, TFG_ERR_ARG, w + "rh_max must be finite and >= 0");
  if (ds->pressure != 0 && ds->pressure != 1) return fail(h, TFG_ERR_ARG, w + "pressure must be 0 or 1");
  *on = ds->lapse_T != 0.0 || ds->grad_P != 0.0 || ds->rh_max > 0.0 || ds->pressure == 1;
  return TFG_OK;
}
// The forcing kernels' terms (ds == NULL: all off) with the handle's model constants.
ForcingDs forcing_ds(const tfg_handle* h, const tfg_downscale* ds) {
  ForcingDs d{};
  if (ds) {
    d.lapse_T = ds->lapse_T;
    d.grad_P = ds->grad_P;
    d.rh_max = ds->rh_max;
    d.pressure = ds->pressure;
  }
  d.negM_g_R = h->dp.negM_g_R;
  d.eps = h->dp.eps;
  d.one_minus_eps = h->dp.one_minus_eps;
  d.satterlund = h->dp.satterlund;
  return d;
}
}  // namespace

int tfg_set_catchment_forcing(tfg_handle* h, int frame0, int nframes, const double* table, int table_on_device,
                              const double* z_ref, const tfg_downscale* ds) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!table) return fail(h, TFG_ERR_ARG, "null table");
  if (frame0 < 0 || nframes < 1 || (int64_t)frame0 + nframes > h->n_frames)
    return fail(h, TFG_ERR_ARG, "catchment forcing: frames outside 0..n_frames");
  bool on = false;
  if (int rc = check_downscale(h, ds, "catchment forcing", &on)) return rc;
  if (on && !z_ref) return fail(h, TFG_ERR_ARG, "catchment forcing: a downscaling term needs z_ref");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t frame_len = (size_t)5 * h->n_catch;  // table entries per frame
  const double* dtab = table;
  const double* dz = on ? z_ref : nullptr;
  StageRing::Slot* s = nullptr;
  if (!table_on_device) {
    // borrowed for this call only, like tfg_set_inputs' src: table | z_ref
    // through the staging ring, one queued copy
    const size_t tbytes = (size_t)nframes * frame_len * 8, bytes = tbytes + (on ? (size_t)h->n_catch * 8 : 0);
    HIPCHK(h, h->in_ring.acquire(bytes, true, &s));
    std::memcpy(s->host.ptr, table, tbytes);
    if (on) std::memcpy(static_cast<char*>(s->host.ptr) + tbytes, z_ref, (size_t)h->n_catch * 8);
    HIPCHK(h, hipMemcpyAsync(s->dev.ptr, s->host.ptr, bytes, hipMemcpyHostToDevice, h->stream));
    dtab = static_cast<const double*>(s->dev.ptr);
    if (on) dz = dtab + (size_t)nframes * frame_len;
  }
  if (h->engine == TFG_F32) {
    // finite-data tracking: a plain gather of a host table leaves in a plane
    // exactly its table row's values (every cell is written), so the row
    // decides; a device table or a downscaled plane is checked lazily
    for (int j = 0; j < nframes; ++j)
      for (int f = 0; f < 5; ++f)  // the table's rows are in BMI order
        h->plane_state[(size_t)(frame0 + j) * kNumForc + kBmiToPlane[f]] =
            (table_on_device || on) ? kUnknown : host_finite_as_f32(table + (size_t)j * frame_len + (size_t)f * h->n_catch, h->n_catch);
  }
  const ForcingDs d = forcing_ds(h, on ? ds : nullptr);
  const bool wide = forcing_wide();
  for (int j0 = 0; j0 < nframes; j0 += kForcingBatch) {
    const int nb = std::min(kForcingBatch, nframes - j0);
    char* fr = h->forc.bytes() + (size_t)(frame0 + j0) * kNumForc * h->n_pad * h->rsz;
    const double* tb = dtab + (size_t)j0 * frame_len;
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      constexpr int V = 16 / (int)sizeof(R);  // cells per lane of the wide form
      auto launch = [&](auto kern, int v) {
        hipLaunchKernelGGL(kern, forcing_blocks(h->n, v), kBlock, 0, h->stream, (R*)fr, h->n_pad, nb, tb, dz,
                           (const R*)h->stat.ptr, h->catch_id, h->n, h->n_catch, d);
      };
      if (wide) { if (on) launch(k_forcing_expand<R, true, V>, V); else launch(k_forcing_expand<R, false, V>, V); }
      else { if (on) launch(k_forcing_expand<R, true, 1>, 1); else launch(k_forcing_expand<R, false, 1>, 1); }
    });
    HIPCHK(h, hipGetLastError());
  }
  if (s) HIPCHK(h, StageRing::commit(*s, h->stream));
  return TFG_OK;
}

int tfg_set_gridded_forcing(tfg_handle* h, int frame0, int nframes, const double* src, int src_on_device,
                            const double* z_src, const tfg_forcing_grid* g, const tfg_downscale* ds) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!src) return fail(h, TFG_ERR_ARG, "gridded forcing: null src");
  if (!g) return fail(h, TFG_ERR_ARG, "gridded forcing: null grid");
  if (frame0 < 0 || nframes < 1 || (int64_t)frame0 + nframes > h->n_frames)
    return fail(h, TFG_ERR_ARG, "gridded forcing: frames outside 0..n_frames");
  if (g->gny < 1 || g->gnx < 1) return fail(h, TFG_ERR_ARG, "gridded forcing: gny and gnx must be >= 1");
  if ((int64_t)g->gny * g->gnx >= ((int64_t)1 << 29))  // k_forcing_regrid's 32-bit byte offsets into a field
    return fail(h, TFG_ERR_ARG, "gridded forcing: a source field must be under 4 GiB (gny * gnx < 2^29)");
  if (g->method != TFG_REGRID_NEAREST && g->method != TFG_REGRID_BILINEAR)
    return fail(h, TFG_ERR_ARG, "gridded forcing: method must be TFG_REGRID_NEAREST or TFG_REGRID_BILINEAR");
  if (!std::isfinite(g->y0) || !std::isfinite(g->x0) || !std::isfinite(g->sy) || !std::isfinite(g->sx))
    return fail(h, TFG_ERR_ARG, "gridded forcing: y0, x0, sy and sx must be finite");
  if (g->row0 < 0) return fail(h, TFG_ERR_ARG, "gridded forcing: row0 must be >= 0");
  bool on = false;
  if (int rc = check_downscale(h, ds, "gridded forcing", &on)) return rc;
  if (on && !z_src) return fail(h, TFG_ERR_ARG, "gridded forcing: a downscaling term needs z_src");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t gnode = (size_t)g->gny * (size_t)g->gnx, frame_len = 5 * gnode;  // source nodes, values per frame
  const double* dsrc = src;
  const double* dz = on ? z_src : nullptr;
  StageRing::Slot* s = nullptr;
  if (!src_on_device) {
    // borrowed for this call only: src | z_src through the staging ring, one queued copy
    const size_t sbytes = (size_t)nframes * frame_len * 8, bytes = sbytes + (on ? gnode * 8 : 0);
    HIPCHK(h, h->in_ring.acquire(bytes, true, &s));
    std::memcpy(s->host.ptr, src, sbytes);
    if (on) std::memcpy(static_cast<char*>(s->host.ptr) + sbytes, z_src, gnode * 8);
    HIPCHK(h, hipMemcpyAsync(s->dev.ptr, s->host.ptr, bytes, hipMemcpyHostToDevice, h->stream));
    dsrc = static_cast<const double*>(s->dev.ptr);
    if (on) dz = dsrc + (size_t)nframes * frame_len;
  }
  if (h->engine == TFG_F32) {
    // finite-data tracking: a plain plane holds values between its field's
    // nodes, so a host field that is finite as fp32 leaves a finite plane; a
    // field with a NaN node may or may not reach a cell, and a device source or
    // a downscaled plane is not looked at: those are checked lazily
    for (int j = 0; j < nframes; ++j)
      for (int f = 0; f < 5; ++f) {  // the source's fields are in BMI order
        const bool finite = !src_on_device && !on && host_finite_as_f32(src + (size_t)j * frame_len + (size_t)f * gnode, (int64_t)gnode) == kOk;
        h->plane_state[(size_t)(frame0 + j) * kNumForc + kBmiToPlane[f]] = finite ? kOk : kUnknown;
      }
  }
  const ForcingDs d = forcing_ds(h, on ? ds : nullptr);
  const bool bilinear = g->method == TFG_REGRID_BILINEAR;
  for (int j0 = 0; j0 < nframes; j0 += kForcingBatch) {
    const int nb = std::min(kForcingBatch, nframes - j0);
    char* fr = h->forc.bytes() + (size_t)(frame0 + j0) * kNumForc * h->n_pad * h->rsz;
    const double* sb = dsrc + (size_t)j0 * frame_len;
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      constexpr int V = 16 / (int)sizeof(R);  // cells per lane: 16-byte stores
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, forcing_blocks(h->n, V), kBlock, 0, h->stream, (R*)fr, h->n_pad, nb, sb, dz,
                           (const R*)h->stat.ptr, h->n, h->nx, *g, d);
      };
      if (on) { if (bilinear) launch(k_forcing_regrid<R, true, true, V>); else launch(k_forcing_regrid<R, true, false, V>); }
      else { if (bilinear) launch(k_forcing_regrid<R, false, true, V>); else launch(k_forcing_regrid<R, false, false, V>); }
    });
    HIPCHK(h, hipGetLastError());
  }
  if (s) HIPCHK(h, StageRing::commit(*s, h->stream));
  return TFG_OK;
}

int tfg_rasterize_polygons(tfg_handle* h, const tfg_polygons* p, int outside_id, int64_t* cells) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!p) return fail(h, TFG_ERR_ARG, "rasterize: null polygons");
  if (p->n_poly < 0 || p->n_rings < 0) return fail(h, TFG_ERR_ARG, "rasterize: n_poly and n_rings must be >= 0");
  if (!p->px || !p->py) return fail(h, TFG_ERR_ARG, "rasterize: null px or py");
  if (!p->poly_ring0 || !p->ring_edge0 || (p->n_poly && (!p->poly_id || !p->poly_box)))
    return fail(h, TFG_ERR_ARG, "rasterize: null table");
  if (outside_id < 0 || outside_id >= h->n_catch) return fail(h, TFG_ERR_ARG, "rasterize: outside_id out of [0, n_catch)");
  if (h->n_catch > kRasterMaxCatch) return fail(h, TFG_ERR_ARG, "rasterize: n_catch > 512 not supported");
  const int64_t tiles = (h->nx + kRasterTile - 1) / kRasterTile;
  if (h->nx > INT32_MAX || h->ny > INT32_MAX || h->ny * tiles > INT32_MAX)
    return fail(h, TFG_ERR_ARG, "rasterize: grid too large (ny * ceil(nx / 1024) must be < 2^31)");
  // everything the kernel indexes with is checked here, before anything is queued or allocated
  if (p->poly_ring0[0] != 0 || p->ring_edge0[0] != 0) return fail(h, TFG_ERR_ARG, "rasterize: offsets must start at 0");
  for (int32_t i = 0; i < p->n_poly; ++i) {
    if (p->poly_id[i] < 0 || p->poly_id[i] >= h->n_catch) return fail(h, TFG_ERR_ARG, "rasterize: polygon id out of [0, n_catch)");
    if (p->poly_ring0[i + 1] < p->poly_ring0[i]) return fail(h, TFG_ERR_ARG, "rasterize: poly_ring0 decreases");
    const int32_t* b = p->poly_box + 4 * (size_t)i;
    if (b[0] < 0 || b[1] < b[0] || b[1] > h->ny || b[2] < 0 || b[3] < b[2] || b[3] > h->nx)
      return fail(h, TFG_ERR_ARG, "rasterize: polygon box outside the grid");
  }
  if (p->poly_ring0[p->n_poly] > p->n_rings) return fail(h, TFG_ERR_ARG, "rasterize: poly_ring0 ends past n_rings");
  for (int32_t k = 0; k < p->n_rings; ++k)
    if (p->ring_edge0[k + 1] < p->ring_edge0[k]) return fail(h, TFG_ERR_ARG, "rasterize: ring_edge0 decreases");
  const int64_t n_edges = p->ring_edge0[p->n_rings];
  if (n_edges && !p->edges) return fail(h, TFG_ERR_ARG, "rasterize: null edges");
  for (int64_t e = 0; e < n_edges; ++e) {
    const double* q = p->edges + 4 * e;
    if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) || !std::isfinite(q[3]))
      return fail(h, TFG_ERR_ARG, "rasterize: non-finite edge");
    if (q[1] == q[3]) return fail(h, TFG_ERR_ARG, "rasterize: horizontal edge (b == d)");
  }
  for (int64_t i = 0; i < h->nx; ++i)
    if (!std::isfinite(p->px[i])) return fail(h, TFG_ERR_ARG, "rasterize: non-finite cell centre");
  for (int64_t i = 0; i < h->ny; ++i)
    if (!std::isfinite(p->py[i])) return fail(h, TFG_ERR_ARG, "rasterize: non-finite cell centre");
  HIPCHK(h, hipSetDevice(h->device));
  // the tables, borrowed for this call only: one block through the staging ring, one queued copy;
  // widest elements first, so every table starts aligned to its element
  const size_t b_edges = (size_t)n_edges * 32, b_px = (size_t)h->nx * 8, b_py = (size_t)h->ny * 8,
               b_re = ((size_t)p->n_rings + 1) * 8, b_box = (size_t)p->n_poly * 16, b_id = (size_t)p->n_poly * 4,
               b_pr = ((size_t)p->n_poly + 1) * 4;
  const size_t o_box = b_edges, o_px = o_box + b_box, o_py = o_px + b_px, o_re = o_py + b_py, o_id = o_re + b_re,
               o_pr = o_id + b_id, bytes = o_pr + b_pr;
  StageRing::Slot* s = nullptr;
  HIPCHK(h, h->in_ring.acquire(bytes, true, &s));
  char* hp = static_cast<char*>(s->host.ptr);
  const char* dp = static_cast<const char*>(s->dev.ptr);
  if (b_edges) std::memcpy(hp, p->edges, b_edges);
  if (b_box) std::memcpy(hp + o_box, p->poly_box, b_box);
  std::memcpy(hp + o_px, p->px, b_px);
  std::memcpy(hp + o_py, p->py, b_py);
  std::memcpy(hp + o_re, p->ring_edge0, b_re);
  if (b_id) std::memcpy(hp + o_id, p->poly_id, b_id);
  std::memcpy(hp + o_pr, p->poly_ring0, b_pr);
  if (cells) HIPCHK(h, reserve_idle(h, h->rd_out_int, (size_t)h->n_catch * 8));
  if (int rc = reserve_zeroed(h, h->catch_id, (size_t)h->n_pad * 4)) return rc;
  HIPCHK(h, hipMemcpyAsync(s->dev.ptr, s->host.ptr, bytes, hipMemcpyHostToDevice, h->stream));
  if (cells) HIPCHK(h, hipMemsetAsync(h->rd_out_int, 0, (size_t)h->n_catch * 8, h->stream));
  RasterTables t;
  t.edges = reinterpret_cast<const double2*>(dp);
  t.poly_box = reinterpret_cast<const int4*>(dp + o_box);
  t.px = reinterpret_cast<const double*>(dp + o_px);
  t.py = reinterpret_cast<const double*>(dp + o_py);
  t.ring_edge0 = reinterpret_cast<const int64_t*>(dp + o_re);
  t.poly_id = reinterpret_cast<const int32_t*>(dp + o_id);
  t.poly_ring0 = reinterpret_cast<const int32_t*>(dp + o_pr);
  t.n_poly = p->n_poly;
  hipLaunchKernelGGL(k_rasterize, (unsigned)(h->ny * tiles), kBlock, 0, h->stream, (int32_t*)h->catch_id, (int32_t)h->ny,
                     (int32_t)h->nx, (int32_t)tiles, t, (int32_t)outside_id, (int32_t)h->n_catch,
                     cells ? reinterpret_cast<unsigned long long*>((int64_t*)h->rd_out_int) : nullptr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, StageRing::commit(*s, h->stream));
  if (cells) {
    HIPCHK(h, hipMemcpyAsync(cells, h->rd_out_int, (size_t)h->n_catch * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return TFG_OK;
}

namespace {

// frame <- src[5][n] (device-visible pointer)
int launch_scatter(tfg_handle* h, int frame, const void* dsrc, int src_dtype, int64_t n) {
  char* fr = h->forc.bytes() + (size_t)frame * kNumForc * h->n_pad * h->rsz;
  by_types(h->engine, src_dtype, [&](auto r, auto s) {
    using R = typename decltype(r)::type;
    using S = typename decltype(s)::type;
    hipLaunchKernelGGL((k_scatter_inputs<R, S>), grid_for(n), 256, 0, h->stream, (R*)fr, (const S*)dsrc, n, h->n_pad);
  });
  HIPCHK(h, hipGetLastError());
  return TFG_OK;
}

// dst[8][n] (device-visible pointer) <- outputs of history slot `hist`
int launch_gather(tfg_handle* h, int hist, void* gdst, int dst_dtype, int64_t n) {
  const char* hs = h->hist.bytes() + (size_t)hist * kNumHist * h->n_pad * h->rsz;
  const int from_state = h->depths_derived ? 0 : 1;
  by_types(h->engine, dst_dtype, [&](auto r, auto d) {
    using R = typename decltype(r)::type;
    using D = typename decltype(d)::type;
    hipLaunchKernelGGL((k_gather_outputs<R, D>), grid_for(n), 256, 0, h->stream, (D*)gdst, (const R*)hs, h->st, n, h->n_pad,
                       from_state);
  });
  HIPCHK(h, hipGetLastError());
  return TFG_OK;
}

}  // namespace

int tfg_get_outputs(tfg_handle* h, int hist, void* dst, int dst_dtype, int64_t n, int dst_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!dst) return fail(h, TFG_ERR_ARG, "null dst");
  if (n != h->n) return fail(h, TFG_ERR_ARG, "n != ny*nx");
  if (hist < 0 || hist >= h->hist_depth) return fail(h, TFG_ERR_ARG, "history slot out of range");
  if (dst_dtype != TFG_F32 && dst_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "dst dtype must be TFG_F32/TFG_F64");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)8 * n * dtype_size(dst_dtype);
  void* gdst = dst;
  if (!dst_on_device) {
    HIPCHK(h, h->out_d.reserve(bytes));  // the call is synchronous: nothing queued still uses them
    HIPCHK(h, h->out_h.reserve(bytes));
    gdst = h->out_d;
  }
  if (int rc = launch_gather(h, hist, gdst, dst_dtype, n)) return rc;
  if (!dst_on_device) {
    HIPCHK(h, hipMemcpyAsync(h->out_h.ptr, h->out_d, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(dst, h->out_h.ptr, bytes);
  }
  return TFG_OK;
}

#ifdef TFG_UPDATE_TIMING
// Diagnostic build only (tests/diagnostics/bmi_many_instances.py): where the
// time of tfg_update goes, summed over calls [ns]: input packing, the launch
// call, waiting for the release flags, output unpacking; [4] = calls.
static double g_upd_ns[5];
extern "C" void tfg_update_timing(double* out) {
  for (int i = 0; i < 5; ++i) out[i] = g_upd_ns[i];
}
#define TFG_TSTAMP(v) const auto v = std::chrono::steady_clock::now()
#define TFG_TACC(i, a, b) (g_upd_ns[i] += std::chrono::duration<double, std::nano>((b) - (a)).count())
#else
#define TFG_TSTAMP(v)
#define TFG_TACC(i, a, b)
#endif

namespace {
// Wait until the `blocks` workgroups of a tfg_update / tfg_update_many launch
// on `stream` have each stored `seq` to their release flag in the mapped block
// (a few microseconds sooner than a stream synchronisation); after ~2 ms fall
// back to the stream wait, which also reports a failed launch.  h (may be
// null) takes the error.
int wait_flags(tfg_handle* h, const char* flags, int blocks, uint32_t seq, hipStream_t stream) {
  const volatile uint32_t* fl = reinterpret_cast<const volatile uint32_t*>(flags);
  const auto t0 = std::chrono::steady_clock::now();
  int done = 0;
  for (int64_t spins = 0; done < blocks; ++spins) {
    while (done < blocks && fl[done] == seq) ++done;
    if (done < blocks && (spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
  if (done == blocks) std::atomic_thread_fence(std::memory_order_acquire);
  else HIPCHK(h, hipStreamSynchronize(stream));
  return TFG_OK;
}
}  // namespace

int tfg_update(tfg_handle* h, int frame, const void* src, int src_dtype, const tfg_uniforms* u, void* dst,
               int dst_dtype, int64_t n) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  TFG_TSTAMP(t_in0);
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!src || !dst) return fail(h, TFG_ERR_ARG, "null src/dst");
  if (n != h->n) return fail(h, TFG_ERR_ARG, "n != ny*nx");
  if (frame < 0 || frame >= h->n_frames) return fail(h, TFG_ERR_ARG, "frame index out of range");
  if (src_dtype != TFG_F32 && src_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "src dtype must be TFG_F32/TFG_F64");
  if (dst_dtype != TFG_F32 && dst_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "dst dtype must be TFG_F32/TFG_F64");
  if (int rc = check_step(h, u, 1)) return rc;
  if (u->frame != frame) return fail(h, TFG_ERR_ARG, "uniforms: frame differs from the input frame");
  HIPCHK(h, hipSetDevice(h->device));
  // One pinned block [forcing kNumForc x n_pad (engine type) | uniforms, step record | outputs 8 x n f64];
  // the call is synchronous, so one block suffices.
  const int64_t np = h->n_pad;
  const size_t in_b = (size_t)kNumForc * np * h->rsz;
  const size_t u_off = (in_b + 255) & ~(size_t)255;
  const size_t out_off = u_off + 256;
  static_assert(stage_bytes(1) <= 256, "the step's uniforms and its table record fit their slot");
  const size_t out_b = (size_t)8 * n * 8;
  const int blocks = fused_blocks(h);
  const size_t flag_off = (out_off + out_b + 255) & ~(size_t)255;
  const size_t total = flag_off + (size_t)blocks * 4;
  if (h->io.mem.cap < total) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->io.reserve(total));  // zeroed: padding cells read zeros, flags start at 0
  }
  char* const io_h = h->io.host();
  char* const io_d = h->io.dev;
  // the step's outputs and flags in the block; its inputs (IoArgs::in) only where k_fused reads them there
  IoArgs io;
  io.out = reinterpret_cast<double*>(io_d + out_off);
  io.flag = reinterpret_cast<uint32_t*>(io_d + flag_off);
  io.seq = h->io.next_seq();
  auto unpack = [&] {  // the block's outputs into dst
    const double* oh = reinterpret_cast<const double*>(io_h + out_off);
    if (dst_dtype == TFG_F64) std::memcpy(dst, oh, out_b);
    else for (int64_t i = 0; i < 8 * n; ++i) static_cast<float*>(dst)[i] = (float)oh[i];
  };
  if (h->engine == TFG_F64 && n == 1) {
    // one catchment (NextGen's per-catchment model): k_cell, inputs and
    // uniforms as kernel arguments, one workgroup of four waves
    CellIo cio;
    cio.u = *u;
    for (int f = 0; f < 5; ++f)
      cio.in[kBmiToPlane[f]] = src_dtype == TFG_F64 ? static_cast<const double*>(src)[f] : (double)static_cast<const float*>(src)[f];
    TFG_TSTAMP(t_c0);
    TFG_TACC(0, t_in0, t_c0);
    if (int rc = prepare_steps(h)) return rc;
    hipLaunchKernelGGL(k_cell, 1, 64 * tfg::kCellWaves, 0, h->stream, step_args(h, 1, io), cio, (const double*)h->geo.ptr,
                       h->catch_id, h->st, h->tot, h->ring, (double*)h->forc.ptr, (double*)h->hist.ptr, h->slab,
                       h->qc_on ? (const double*)h->qc.ptr : nullptr, h->depths_derived ? 0 : 1);
    HIPCHK(h, hipGetLastError());
    h->depths_derived = true;
    h->last_hist = u->hist;
    TFG_TSTAMP(t_c1);
    TFG_TACC(1, t_c0, t_c1);
    if (int rc = wait_flags(h, io_h + flag_off, 1, io.seq, h->stream)) return rc;
    TFG_TSTAMP(t_c2);
    TFG_TACC(2, t_c1, t_c2);
    unpack();
    TFG_TSTAMP(t_c3);
    TFG_TACC(3, t_c2, t_c3);
#ifdef TFG_UPDATE_TIMING
    g_upd_ns[4] += 1;
#endif
    return TFG_OK;
  }
  // BMI order -> the frame's planes, converted to the engine type
  by_types(h->engine, src_dtype, [&](auto r, auto s) {
    using R = typename decltype(r)::type;
    using S = typename decltype(s)::type;
    for (int f = 0; f < 5; ++f)
      std::copy_n(static_cast<const S*>(src) + (size_t)f * n, n, reinterpret_cast<R*>(io_h) + (size_t)kBmiToPlane[f] * np);
  });
  std::memcpy(io_h + u_off, u, sizeof(tfg_uniforms));
  step_table(h, u, 1, reinterpret_cast<StepAddr*>(io_h + u_off + sizeof(tfg_uniforms)), true);
  if (h->engine == TFG_F32) {  // finite-data status of the step's inputs, as the kernel reads them
    io.in_state = kOk;
    for (int f = 0; f < 5; ++f)
      if (host_finite_as_f32(reinterpret_cast<const float*>(io_h + (size_t)kBmiToPlane[f] * np * h->rsz), n) != kOk) io.in_state = kDirty;
  }
  TFG_TSTAMP(t_in1);
  TFG_TACC(0, t_in0, t_in1);
  io.in = io_d;
  const tfg_uniforms* d_u = reinterpret_cast<const tfg_uniforms*>(io_d + u_off);
  if (int rc = launch_steps(h, d_u, table_of(d_u, 1), nullptr, u, 1, io)) return rc;
  if (h->engine == TFG_F32)  // the kernel stored the inputs into the frame
    std::fill_n(h->plane_state.begin() + (size_t)frame * kNumForc, kNumForc, io.in_state);
  TFG_TSTAMP(t_l1);
  TFG_TACC(1, t_in1, t_l1);
  if (int rc = wait_flags(h, io_h + flag_off, blocks, io.seq, h->stream)) return rc;
  TFG_TSTAMP(t_w1);
  TFG_TACC(2, t_l1, t_w1);
  unpack();
  TFG_TSTAMP(t_o1);
  TFG_TACC(3, t_w1, t_o1);
#ifdef TFG_UPDATE_TIMING
  g_upd_ns[4] += 1;
#endif
  return TFG_OK;
}

namespace {
// tfg_update_many's pinned, device-mapped block of one device:
// [jobs m x CellJob | outputs m x 8 f64 | release flags m x u32].  Calls are
// synchronous, so one block per device serves every call, under its mutex.
struct ManyBlock {
  std::mutex mu;
  MappedBlock io;
};
constexpr int kMaxDevices = 64;
// never destroyed (as tfg_shared_stream's streams): no HIP call during static destruction
ManyBlock* const g_many = new ManyBlock[kMaxDevices];
}  // namespace

int tfg_update_many(tfg_handle* const* hs, int m, const double* const* src, const tfg_uniforms* const* u,
                    double* const* dst) {
  for (int i = 0; hs && i < m; ++i)
    if (int rc_ = api_sync(hs[i])) return rc_;  // after a split launch's second part
  if (m <= 0) return TFG_OK;
  if (!hs || !src || !u || !dst) return fail(nullptr, TFG_ERR_ARG, "tfg_update_many: null argument");
  tfg_handle* h0 = hs[0];
  if (!h0) return fail(nullptr, TFG_ERR_ARG, "tfg_update_many: null handle 0");
  if (h0->device < 0 || h0->device >= kMaxDevices) return fail(nullptr, TFG_ERR_ARG, "tfg_update_many: device id");
  for (int i = 0; i < m; ++i) {
    tfg_handle* h = hs[i];
    const std::string at = "tfg_update_many: handle " + std::to_string(i) + ": ";
    if (!h || !src[i] || !u[i] || !dst[i]) return fail(nullptr, TFG_ERR_ARG, at + "null handle/src/uniforms/dst");
    if (h->engine != TFG_F64 || h->n != 1) return fail(nullptr, TFG_ERR_ARG, at + "not a one-cell TFG_F64 handle");
    if (h->device != h0->device || h->stream != h0->stream)
      return fail(nullptr, TFG_ERR_ARG, at + "every handle must be on one device and share one stream (tfg_shared_stream)");
    if (int rc = check_step(h, u[i], 1)) return fail(nullptr, rc, at + h->err);
  }
  {  // one step per handle per launch: a handle listed twice would race with itself
    std::vector<const tfg_handle*> v(hs, hs + m);
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) != v.end())
      return fail(nullptr, TFG_ERR_ARG, "tfg_update_many: a handle is listed twice");
  }
  ManyBlock& B = g_many[h0->device];
  std::lock_guard<std::mutex> lock(B.mu);
  HIPCHK(nullptr, hipSetDevice(h0->device));
  const size_t job_b = (size_t)m * sizeof(CellJob);
  const size_t out_off = (job_b + 255) & ~(size_t)255;
  const size_t flag_off = (out_off + (size_t)m * 64 + 255) & ~(size_t)255;
  const size_t total = flag_off + (size_t)m * 4;
  if (B.io.mem.cap < total)  // calls are synchronous: no launch still uses the block
    HIPCHK(nullptr, B.io.reserve(std::max(total, B.io.mem.cap * 2)));
  char* const io_h = B.io.host();
  char* const io_d = B.io.dev;
  CellJob* jobs = reinterpret_cast<CellJob*>(io_h);
  for (int i = 0; i < m; ++i) {
    tfg_handle* h = hs[i];
    if (int rc = prepare_steps(h)) return fail(nullptr, rc, "tfg_update_many: " + h->err);
    CellJob& j = jobs[i];
    j.p = h->dp;
    j.u = *u[i];
    for (int f = 0; f < 5; ++f) j.in[kBmiToPlane[f]] = src[i][f];
    j.geo = (const double*)h->geo.ptr;
    j.catch_id = h->catch_id;
    j.st = h->st;
    j.tot = h->tot;
    j.ring = h->ring;
    j.forc = (double*)h->forc.ptr;
    j.hist = (double*)h->hist.ptr;
    j.slab = h->slab;
    j.qc = h->qc_on ? (const double*)h->qc.ptr : nullptr;
    j.n_pad = h->n_pad;
    j.read_depths = h->depths_derived ? 0 : 1;
    j.pad_ = 0;
  }
  const uint32_t seq = B.io.next_seq();
  hipLaunchKernelGGL(k_cell_many, m, 64 * tfg::kCellWaves, 0, h0->stream, reinterpret_cast<const CellJob*>(io_d),
                     reinterpret_cast<double*>(io_d + out_off), reinterpret_cast<uint32_t*>(io_d + flag_off), seq);
  HIPCHK(nullptr, hipGetLastError());
  for (int i = 0; i < m; ++i) {
    hs[i]->depths_derived = true;
    hs[i]->last_hist = u[i]->hist;
  }
  if (int rc = wait_flags(nullptr, io_h + flag_off, m, seq, h0->stream)) return rc;
  const double* oh = reinterpret_cast<const double*>(io_h + out_off);
  for (int i = 0; i < m; ++i) std::memcpy(dst[i], oh + (size_t)i * 8, 64);
  return TFG_OK;
}

int tfg_terrain_from_dem(tfg_handle* h, double dx, double dy, const void* halo_north, const void* halo_south,
                         int halo_dtype, int halo_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!(dx > 0) || !(dy > 0)) return fail(h, TFG_ERR_ARG, "dx and dy must be > 0");
  if (halo_dtype != TFG_F32 && halo_dtype != TFG_F64) return fail(h, TFG_ERR_ARG, "halo dtype must be TFG_F32/TFG_F64");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t nx = h->nx, ny = h->ny;
  HIPCHK(h, h->halo.reserve((size_t)2 * nx * 8));
  const size_t rs = h->rsz;
  const char* el = h->stat.bytes();  // TFG_ST_ELEV plane
  // a missing halo replicates the shard's own edge row (domain boundary)
  const void* src[2] = {halo_north, halo_south};
  for (int k = 0; k < 2; ++k) {
    if (src[k]) {
      int rc = upload(h, h->halo + k * nx, TFG_F64, src[k], halo_dtype, nx, halo_on_device);
      if (rc) return rc;
    } else {
      const int64_t row = k == 0 ? 0 : ny - 1;
      int rc = upload(h, h->halo + k * nx, TFG_F64, el + row * nx * rs, h->engine, nx, 1);
      if (rc) return rc;
    }
  }
  char* st = h->stat.bytes();
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL((k_terrain<R>), grid_for(h->n), 256, 0, h->stream, (const R*)st, h->halo, (R*)(st + h->n_pad * rs),
                       (R*)(st + 2 * h->n_pad * rs), ny, nx, 1.0 / (8.0 * dx), 1.0 / (8.0 * dy));
  });
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->geo_dirty = true;
  h->slope_invalid = false;  // tan(beta) >= 0 always maps into [0, pi/2)
  return TFG_OK;
}


namespace {
// Ice-flow halos into h->flow_halo; FlowGrid over this shard.
int flow_setup(tfg_handle* h, const double* hn, const double* hs, int on_dev, FlowGrid& g) {
  if (!h->initialised) return fail(h, TFG_ERR_STATE, "tfg_init_state() has not been called");
  const int64_t nx = h->nx;
  HIPCHK(h, h->flow_halo.reserve((size_t)4 * nx * 8));
  if (hn) HIPCHK(h, hipMemcpyAsync(h->flow_halo, hn, (size_t)2 * nx * 8, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  if (hs) HIPCHK(h, hipMemcpyAsync(h->flow_halo + 2 * nx, hs, (size_t)2 * nx * 8, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  g.elev = h->stat;
  g.iwe = h->st + S_HIWE * h->n_pad;
  g.hn = hn ? h->flow_halo : nullptr;
  g.hs = hs ? h->flow_halo + 2 * nx : nullptr;
  g.ny = h->ny;
  g.nx = nx;
  g.wi = h->dp.wi;
  return TFG_OK;
}
}  // namespace

int tfg_ice_flow_edges(tfg_handle* h, double* first, double* last, int on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !first || !last) return fail(h, TFG_ERR_ARG, "null argument");
  HIPCHK(h, hipSetDevice(h->device));
  FlowGrid g;
  if (int rc = flow_setup(h, nullptr, nullptr, 0, g)) return rc;
  const int64_t nx = h->nx;
  HIPCHK(h, h->flow_edges.reserve((size_t)4 * nx * 8));
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL((k_ice_flow_edges<R>), grid_for(nx), 256, 0, h->stream, g, h->flow_edges, h->flow_edges + 2 * nx);
  });
  HIPCHK(h, hipGetLastError());
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHK(h, hipMemcpyAsync(first, h->flow_edges, (size_t)2 * nx * 8, k, h->stream));
  HIPCHK(h, hipMemcpyAsync(last, h->flow_edges + 2 * nx, (size_t)2 * nx * 8, k, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

int tfg_ice_flow_dmax(tfg_handle* h, double dx, double dy, const double* halo_north, const double* halo_south,
                      int halo_on_device, double* dmax) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !dmax) return fail(h, TFG_ERR_ARG, "null argument");
  if (!(dx > 0) || !(dy > 0)) return fail(h, TFG_ERR_ARG, "dx and dy must be > 0");
  HIPCHK(h, hipSetDevice(h->device));
  FlowGrid g;
  if (int rc = flow_setup(h, halo_north, halo_south, halo_on_device, g)) return rc;
  const dim3 fgrid((unsigned)((h->nx + kFlowTX - 1) / kFlowTX), (unsigned)((h->ny + kFlowRows - 1) / kFlowRows));
  if (fgrid.y > 65535u) return fail(h, TFG_ERR_ARG, "ice flow: too many rows for one shard");
  const int64_t gb = (int64_t)fgrid.x * fgrid.y;
  const FlowTiles ft = flow_tiles(h->nx, (int)fgrid.y);
  const FlowK fk = flow_constants(1.0, dx, dy, h->dp.wi, h->flow_gamma);  // dt unused by the bound
  HIPCHK(h, h->flow_red.reserve((size_t)gb * 8));  // the grid never changes
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL((k_ice_flow<R, true>), flow_blocks(ft), kFlowTX, 0, h->stream, g, fk, h->flow_red, 0, 1, nullptr, ft);
  });
  HIPCHK(h, hipGetLastError());
  std::vector<double> bm(gb);
  HIPCHK(h, hipMemcpyAsync(bm.data(), h->flow_red, (size_t)gb * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double m = 0.0;
  for (double v : bm) m = std::max(m, v);
  *dmax = m;
  return TFG_OK;
}

int tfg_ice_flow_step(tfg_handle* h, double dt_years, double dx, double dy, const double* halo_north,
                      const double* halo_south, int halo_on_device, int part) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!(dx > 0) || !(dy > 0) || !(dt_years > 0)) return fail(h, TFG_ERR_ARG, "dt, dx and dy must be > 0");
  if (part != TFG_FLOW_ALL && part != TFG_FLOW_INTERIOR && part != TFG_FLOW_EDGES)
    return fail(h, TFG_ERR_ARG, "part must be TFG_FLOW_ALL, TFG_FLOW_INTERIOR or TFG_FLOW_EDGES");
  if (part == TFG_FLOW_INTERIOR && (halo_north || halo_south))
    return fail(h, TFG_ERR_ARG, "the interior part takes no halo rows");
  HIPCHK(h, hipSetDevice(h->device));
  FlowGrid g;
  if (int rc = flow_setup(h, halo_north, halo_south, halo_on_device, g)) return rc;
  HIPCHK(h, h->wtmp.reserve((size_t)h->n_pad * 8));
  const int64_t strips = (h->ny + kFlowRows - 1) / kFlowRows;
  if (strips > 65535) return fail(h, TFG_ERR_ARG, "ice flow: too many rows for one shard");
  const FlowK fk = flow_constants(dt_years, dx, dy, h->dp.wi, h->flow_gamma);
  // strips [first, first + count*step) by `step`: all of them, the interior
  // ones (no halo row read), or the first and last (the halo readers)
  int first = 0, count = (int)strips, step = 1;
  if (part == TFG_FLOW_INTERIOR) { first = 1; count = (int)std::max<int64_t>(strips - 2, 0); }
  if (part == TFG_FLOW_EDGES) { count = strips > 1 ? 2 : 1; step = (int)std::max<int64_t>(strips - 1, 1); }
  // h_ice (not read by the flow kernels) goes straight to the state plane; the
  // new h_iwe goes to scratch, since neighbouring strips still read the old one
  double* ice = h->st + S_HICE * h->n_pad;
  if (count > 0) {
    const FlowTiles ft = flow_tiles(h->nx, count);
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      hipLaunchKernelGGL((k_ice_flow<R, false>), flow_blocks(ft), kFlowTX, 0, h->stream, g, fk, h->wtmp, first, step, ice, ft);
    });
    HIPCHK(h, hipGetLastError());
  }
  if (part == TFG_FLOW_INTERIOR) return TFG_OK;  // queued; the edges part commits
  hipLaunchKernelGGL(k_flow_commit<false>, grid_for(h->n), 256, 0, h->stream, h->st, h->wtmp, h->n, h->n_pad, h->dp.wi);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

int tfg_ice_flow_run(tfg_handle* h, double dt_years, double dx, double dy, int n_sub) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!(dx > 0) || !(dy > 0) || !(dt_years > 0) || n_sub < 1) return fail(h, TFG_ERR_ARG, "dt, dx, dy and n_sub must be > 0");
  HIPCHK(h, hipSetDevice(h->device));
  FlowGrid g;
  if (int rc = flow_setup(h, nullptr, nullptr, 0, g)) return rc;
  HIPCHK(h, h->wtmp.reserve((size_t)h->n_pad * 8));
  const int64_t strips = (h->ny + kFlowRows - 1) / kFlowRows;
  if (strips > 65535) return fail(h, TFG_ERR_ARG, "ice flow: too many rows for one shard");
  const FlowK fk = flow_constants(dt_years / n_sub, dx, dy, h->dp.wi, h->flow_gamma);
  const FlowTiles ft = flow_tiles(h->nx, (int)strips);
  // ping-pong between the state plane and the scratch plane: a sub-step that
  // lands in the state plane writes h_ice with it, so only an odd count needs
  // the commit pass at the end
  double* plane = h->st + S_HIWE * h->n_pad;
  double* ice = h->st + S_HICE * h->n_pad;
  for (int k = 0; k < n_sub; ++k) {
    const bool to_state = (k & 1) != 0;
    g.iwe = to_state ? h->wtmp : plane;
    double* dst = to_state ? plane : h->wtmp;
    by_type(h->engine, [&](auto t) {
      using R = typename decltype(t)::type;
      hipLaunchKernelGGL((k_ice_flow<R, false>), flow_blocks(ft), kFlowTX, 0, h->stream, g, fk, dst, 0, 1,
                         to_state ? ice : nullptr, ft);
    });
    HIPCHK(h, hipGetLastError());
  }
  if (n_sub & 1)
    hipLaunchKernelGGL(k_flow_commit<true>, grid_for(h->n), 256, 0, h->stream, h->st, h->wtmp, h->n, h->n_pad, h->dp.wi);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

namespace {
// Conduction halos into h->cond_halo; the CondGrid of this shard.
int cond_setup(tfg_handle* h, const double* hn, const double* hs, int on_dev, tfg::CondGrid& g) {
  if (!h->initialised) return fail(h, TFG_ERR_STATE, "tfg_init_state() has not been called");
  const int64_t nx = h->nx, np = h->n_pad;
  HIPCHK(h, h->cond_halo.reserve((size_t)8 * nx * 8));
  const hipMemcpyKind k = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (hn) HIPCHK(h, hipMemcpyAsync(h->cond_halo, hn, (size_t)4 * nx * 8, k, h->stream));
  if (hs) HIPCHK(h, hipMemcpyAsync(h->cond_halo + 4 * nx, hs, (size_t)4 * nx * 8, k, h->stream));
  static_assert(S_HIWE == S_HSWE + 1 && S_ECCS == S_HSWE + 2 && S_ECCI == S_HSWE + 3,
                "k_conduction reads h_swe, h_iwe, Eccs, Ecci as consecutive planes");
  g.st = h->st + S_HSWE * np;
  g.hn = hn ? h->cond_halo : nullptr;
  g.hs = hs ? h->cond_halo + 4 * nx : nullptr;
  g.ny = h->ny;
  g.nx = nx;
  g.n_pad = np;
  g.ws = h->dp.ws;
  g.wi = h->dp.wi;
  g.T0 = h->dp.T0;
  g.inv_cs = h->inv_cs;
  g.inv_ci = h->inv_ci;
  return TFG_OK;
}
}  // namespace

int tfg_conduction_edges(tfg_handle* h, double* first, double* last, int on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h || !first || !last) return fail(h, TFG_ERR_ARG, "null argument");
  HIPCHK(h, hipSetDevice(h->device));
  tfg::CondGrid g;
  if (int rc = cond_setup(h, nullptr, nullptr, 0, g)) return rc;
  const int64_t nx = h->nx;
  HIPCHK(h, h->cond_edges.reserve((size_t)8 * nx * 8));
  hipLaunchKernelGGL(tfg::k_conduction_edges, grid_for(nx), 256, 0, h->stream, g, h->cond_edges, h->cond_edges + 4 * nx);
  HIPCHK(h, hipGetLastError());
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHK(h, hipMemcpyAsync(first, h->cond_edges, (size_t)4 * nx * 8, k, h->stream));
  HIPCHK(h, hipMemcpyAsync(last, h->cond_edges + 4 * nx, (size_t)4 * nx * 8, k, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TFG_OK;
}

int tfg_conduction_update(tfg_handle* h, double k_snow, double k_ice, double dx, double dy, double q_ground,
                          const double* halo_north, const double* halo_south, int halo_on_device) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  if (!(dx > 0) || !(dy > 0)) return fail(h, TFG_ERR_ARG, "dx and dy must be > 0");
  if (!(k_snow >= 0) || !(k_ice >= 0)) return fail(h, TFG_ERR_ARG, "conductivities must be >= 0");
  // every argument check before cond_setup queues copies from the caller's halo rows
  if (!std::isfinite(q_ground)) return fail(h, TFG_ERR_ARG, "ground heat flux must be finite");
  const int64_t gx = (h->nx + tfg::kCondOut - 1) / tfg::kCondOut, strips = (h->ny + tfg::kCondRows - 1) / tfg::kCondRows;
  const int64_t per_xcd = (gx * strips + 7) / 8;
  if (8 * per_xcd > 0x7fffffff) return fail(h, TFG_ERR_ARG, "conduction: grid too large");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = ensure_qc(h)) return rc;
  tfg::CondGrid g;
  if (int rc = cond_setup(h, halo_north, halo_south, halo_on_device, g)) return rc;
  const tfg::CondK K = {k_snow / (dx * dx), k_snow / (dy * dy), k_ice * h->h_active / (dx * dx),
                        k_ice * h->h_active / (dy * dy), q_ground};
  by_type(h->engine, [&](auto t) {
    using R = typename decltype(t)::type;
    hipLaunchKernelGGL((tfg::k_conduction<R>), (unsigned)(8 * per_xcd), tfg::kCondTX, 0, h->stream, g, K, (R*)h->qc.ptr,
                       (int)gx, (int)strips, (int)per_xcd);
  });
  HIPCHK(h, hipGetLastError());
  // the halo rows are the caller's: finish reading them before returning
  if (halo_north || halo_south) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->qc_on = true;
  // Qc of a finite state is finite; a neighbour's halo rows are not checked here
  h->qc_state = (h->state_state == kOk && !halo_north && !halo_south) ? kOk : kUnknown;
  return TFG_OK;
}

int tfg_conduction_off(tfg_handle* h) {
  if (int rc_ = api_sync(h)) return rc_;  // after a split launch's second part
  if (!h) return fail(nullptr, TFG_ERR_ARG, "null handle");
  h->qc_on = false;
  if (h->qc) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->qc, 0, (size_t)h->n_pad * h->rsz, h->stream));
  }
  return TFG_OK;
}

const char* tfg_last_error(const tfg_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

}  // extern "C"
