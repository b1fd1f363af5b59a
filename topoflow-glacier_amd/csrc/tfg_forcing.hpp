// tfg_forcing.hpp -- per-catchment forcing spread over the grid, device side (gfx950).
//
// Included by tfg_engine.hip after the frame layout (kNumForc, F_*), kBlock and
// the physics' device functions; the C ABI entry point
// (tfg_set_catchment_forcing) lives there.
#pragma once

// ---------------------------------------------------------------------------
// Catchment forcing (tfg_set_catchment_forcing): a caller of the reference
// sets five forcing values per catchment and step
// (examples/run_topoflow_glacier.py:63-71).  On a grid with a catchment-id
// raster each cell takes its catchment's values, optionally corrected for the
// cell's height above the catchment's reference elevation.  The reference has
// no such term (it is one cell per catchment), so the rule is pinned by its
// numpy restatement (tests/downscale_ref.py).  For cell i with c = catch_id[i]
// (0 without a raster), dz = elev[i] - z_ref[c] and the table values X_c of a
// frame, all in fp64 and rounded once to the frame's element type:
//   uz     = uz_c
//   T_air  = T_c + lapse_T dz
//   P      = P_c max(0, 1 + grad_P dz)
//   P_air  = P_air_c exp(-M g dz / (R (T_c + 273.15)))   (pressure == 1; the
//            model's barometric form, :519-556, as a ratio between two heights)
//   Hum_sp = q_c, or with rh_max > 0 capped so that the cell's relative
//            humidity stays at or under rh_max:
//              e     = q P_air / (eps + (1 - eps) q) / 100      [mbar] (:809-826)
//              e_cap = rh_max e_sat(T_air)                       (forcing_e_sat)
//              q     = eps e_cap / (P_air / 100 - (1 - eps) e_cap)   where e > e_cap
// With every term off (DS = false) it is a plain gather, without a
// transcendental: each cell gets exactly its catchment's value, converted once.
//
// Shape: a pure write stream, 5 sizeof(R) bytes per cell and frame, against
// 4 + sizeof(R) bytes read per cell (the id and the elevation) once per batch
// of up to kForcingBatch frames.  Workgroups own whole, aligned chunks of
// kBlock cells, in tiles of V chunks: a lane holds V consecutive cells (a wave
// 64 V of them), loads their ids and elevations once, forms dz and what else
// does not depend on the frame once, and then produces every frame of the
// batch.  A plane is addressed as a wave-uniform base (frame, plane, the wave's
// first cell) plus the lane's offset, and stored V cells at a time: with V = 4
// (float) or 2 (double) one 16-byte store per lane and plane, 1 KiB per wave
// instruction.  Cells at or past n load cell n-1 (an in-bounds address) and
// store nothing: the plane padding [n, n_pad) stays as it is.
//
// The table [frames][5][n_catch] fp64 is tiny (at most 8 * 5 * 512 * 8 B per
// batch) and is served from the caches, not from LDS: a wave whose cells share
// one id -- the normal case on a divide raster, and every wave without a
// raster -- reads its five entries per frame at a wave-uniform address (the id
// through readfirstlane: scalar loads, once per wave), and a wave with several
// ids gathers them per lane.  No atomics, no LDS, no dependence between the
// frames of a call: a frame's planes are the same bit for bit whichever call
// and batch position produced them.  A NaN table entry reaches only what is
// computed from it: on a plain gather its own plane in its own catchment and
// frame.
constexpr int kForcingBatch = 8;  // frames per launch

// Workgroups of a k_forcing_expand launch: at most 16 per CU with one cell per
// lane, 8 with several (the same cells per CU in flight either way).
inline int forcing_blocks(int64_t n, int v) {
  const int64_t tile = (int64_t)kBlock * v;
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + tile - 1) / tile, v == 1 ? 4096 : 2048));
}

// The downscaling terms with the model constants they need (kernel argument).
struct ForcingDs {
  double lapse_T, grad_P, rh_max;
  double negM_g_R;            // -M g / R_star (DevParams)
  double eps, one_minus_eps;  // :817
  int32_t pressure, satterlund;
};

namespace tfg {

// Saturation vapour pressure over the air temperature [mbar] in the handle's
// configured form (:788-802), from the functions the fp64 step evaluates it
// with (cell_step_exact's e_sat_surf).
__device__ __forceinline__ double forcing_e_sat(bool satterlund, double T) {
#pragma clang fp contract(off)
  double e;
  if (!satterlund) e = 0.611 * exp_k(fdiv(17.3 * T, T + 237.3));
  else e = div_r(pow(opaque(10.0), 11.4 - fdiv(2353.0, T + 273.15)), 1.0 / 1000.0);
  return e * 10.0;
}

// One cell of one frame.  t: the catchment's table values in tfg_set_inputs
// order (P_air, Hum_sp, P, T_air, uz); o: the cell's values in frame-plane
// order (F_*).  pfac = max(0, 1 + grad_P dz), dT = lapse_T dz and
// xP = -M g dz / R do not depend on the frame.
template <bool DS>
__device__ __forceinline__ void forcing_cell(const ForcingDs& d, const double (&t)[5], double pfac, double dT, double xP,
                                             double (&o)[kNumForc]) {
#pragma clang fp contract(off)
  if constexpr (!DS) {
    o[F_PA] = t[0];
    o[F_Q] = t[1];
    o[F_P] = t[2];
    o[F_T] = t[3];
    o[F_UZ] = t[4];
  } else {
    const double T = t[3] + dT;
    double pa = t[0];
    if (d.pressure) pa = pa * exp_k(fdiv(xP, t[3] + 273.15));
    double q = t[1];
    if (d.rh_max > 0.0) {
      const double e = div_r(fdiv(q * pa, d.eps + d.one_minus_eps * q), 1.0 / 100.0);
      const double e_cap = d.rh_max * forcing_e_sat(d.satterlund != 0, T);
      const double q_cap = tfg_fm::fdiv_z(d.eps * e_cap, div_r(pa, 1.0 / 100.0) - d.one_minus_eps * e_cap);
      q = e > e_cap ? q_cap : q;
    }
    o[F_PA] = pa;
    o[F_Q] = q;
    o[F_P] = t[2] * pfac;
    o[F_T] = T;
    o[F_UZ] = t[4];
  }
}

}  // namespace tfg

// fr: plane 0 of the batch's first frame (frames are consecutive, kNumForc *
// n_pad elements apart); tab: [nb][5][n_catch] of the same frames; nb <=
// kForcingBatch.  z_ref [n_catch] and elev [n_pad] are read only with DS;
// catch_id may be null (every cell in catchment 0).
template <class R, bool DS, int V>
__global__ __launch_bounds__(kBlock) void k_forcing_expand(R* __restrict__ fr, int64_t n_pad, int nb,
                                                           const double* __restrict__ tab,
                                                           const double* __restrict__ z_ref,
                                                           const R* __restrict__ elev,
                                                           const int32_t* __restrict__ catch_id, int64_t n, int n_catch,
                                                           ForcingDs d) {
  constexpr int kTile = kBlock * V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ntiles = (n + kTile - 1) / kTile;
  const int64_t t0 = (int64_t)blockIdx.x * ntiles / gridDim.x, t1 = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  const int64_t fstride = (int64_t)kNumForc * n_pad;
  const int loff = lane * V;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t wbase = t * kTile + wave * (64 * V);  // the wave's first cell: wave-uniform
    const int64_t i0 = wbase + loff;
    // once per cell and batch: the id, and with DS what hangs on dz alone
    int c[V];
    double pfac[V], dT[V], xP[V];
    bool same = true;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t il = i0 + j < n ? i0 + j : n - 1;
      c[j] = catch_id ? catch_id[il] : 0;
      if constexpr (DS) {
#pragma clang fp contract(off)
        const double dz = (double)elev[il] - z_ref[c[j]];
        pfac[j] = fmax(0.0, 1.0 + d.grad_P * dz);
        dT[j] = d.lapse_T * dz;
        xP[j] = d.negM_g_R * dz;
      } else {
        pfac[j] = 1.0;
        dT[j] = xP[j] = 0.0;
      }
    }
    const int cf = __builtin_amdgcn_readfirstlane(c[0]);
#pragma unroll
    for (int j = 0; j < V; ++j) same &= c[j] == cf;
    const bool one_id = __all(same);  // one id in the wave: its table entries at a uniform address
    const bool full = i0 + V <= n;
    // the gather's frames are unrolled (their stores and table loads overlap);
    // the downscaled form keeps one frame's arithmetic live at a time
    auto frame = [&](int s) {
      const double* __restrict__ ts = tab + (int64_t)s * 5 * n_catch;
      R o[kNumForc][V];  // rounded once, as each cell is finished
      auto cell = [&](const double (&tv)[5], int j) {
        double x[kNumForc];
        tfg::forcing_cell<DS>(d, tv, pfac[j], dT[j], xP[j], x);
#pragma unroll
        for (int p = 0; p < kNumForc; ++p) o[p][j] = (R)x[p];
      };
      if (one_id) {
        double tv[5];
#pragma unroll
        for (int v = 0; v < 5; ++v) tv[v] = ts[(int64_t)v * n_catch + cf];
#pragma unroll
        for (int j = 0; j < V; ++j) cell(tv, j);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          double tv[5];
#pragma unroll
          for (int v = 0; v < 5; ++v) tv[v] = ts[(int64_t)v * n_catch + c[j]];
          cell(tv, j);
        }
      }
      R* const fp = fr + s * fstride + wbase;  // wave-uniform plane base, lane offset loff
#pragma unroll
      for (int p = 0; p < kNumForc; ++p) {
        R* const q = fp + p * n_pad + loff;
        if constexpr (V == 1) {
          if (full) q[0] = o[p][0];
        } else {
          typedef R vec __attribute__((ext_vector_type(V)));
          if (full) {
            vec x;
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = o[p][j];
            *reinterpret_cast<vec*>(q) = x;
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
              if (i0 + j < n) q[j] = o[p][j];
          }
        }
      }
    };
    if constexpr (DS) {
#pragma unroll 1
      for (int s = 0; s < nb; ++s) frame(s);
    } else {
#pragma unroll
      for (int s = 0; s < kForcingBatch; ++s)
        if (s < nb) frame(s);
    }
  }
}
