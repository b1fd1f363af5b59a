// tfg_forcing.hpp -- forcing frames produced on the device (gfx950): a
// per-catchment table spread over the grid (k_forcing_expand), and fields on a
// regular source grid interpolated onto it (k_forcing_regrid).
//
// Included by tfg_engine.hip after the frame layout (kNumForc, F_*), kBlock and
// the physics' device functions; the C ABI entry points
// (tfg_set_catchment_forcing, tfg_set_gridded_forcing) live there.
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

// ---------------------------------------------------------------------------
// Gridded forcing (tfg_set_gridded_forcing): the five inputs on a regular
// source grid far coarser than the model's (AORC, WRF), interpolated onto the
// model grid, optionally with the elevation terms above.  The reference has no
// such term; the rule is pinned by its numpy restatement (tests/regrid_ref.py).
// Source node (j, i) sits at source-grid coordinate (j, i).  For local cell
// (r, c) of a shard whose first row is global row row0, all in fp64 without
// contraction and rounded once to the frame's element type:
//   y = y0 + sy (row0 + r),  yc = min(max(y, 0), gny - 1)      (x alike, from c)
// The clamp comes before the conversion to an integer: outside the source the
// edge value is held and no index can overflow.
//   bilinear  j0 = min(floor(yc), max(gny - 2, 0)), j1 = min(j0 + 1, gny - 1),
//             wy = yc - j0 (i0, i1, wx alike); vertically first:
//               west = a[j0][i0] + wy (a[j1][i0] - a[j0][i0])
//               east = a[j0][i1] + wy (a[j1][i1] - a[j0][i1])
//               v    = west + wx (east - west)
//   nearest   v = a[floor(yc + 0.5)][floor(xc + 0.5)]           (ties go up)
// Without a term the five interpolated fields are the cell's values.  With one,
// they take the place of a catchment's table values and the interpolated z_src
// that of z_ref: dz = elev - z, then forcing_cell<true> as above.  A NaN node
// reaches exactly the cells whose stencil holds it (a weight of 0 does not stop
// it: 0 NaN = NaN), in its own frame and variable plus what forcing_cell
// derives from it.
//
// Shape: k_forcing_expand's write stream and tiling (a lane holds V consecutive
// cells, 16-byte stores, cells at or past n load in-bounds addresses and store
// nothing).  What does not depend on the frame is formed once per cell and
// batch: the stencil's node offsets and weights, and with DS the interpolated
// z_src, dz, pfac, dT and xP.  The source (gny gnx 40 bytes per frame) is
// served from L2 and the Infinity Cache, and it is the gathers' issue, not
// HBM, that bounds the kernel: four fp64 gathers per value against one store
// per four values.  So a wave that lies in one model row over at most 64
// source columns -- the normal case under a coarser source -- forms each
// source column's vertical lerp once, in the lane that owns the column (two
// loads per lane and field), and its cells read their west and east column
// values from those lanes; any other wave (a finer source, a wave straddling
// a row end) gathers its four nodes per cell.  Both evaluate the same
// expression and give the same bits.  Measured at 8192^2 under 257^2 nodes,
// 24 fp32 frames: 10.0 ms bilinear against 16.1 ms with per-lane gathers
// alone, 7.2 against 9.6 ms nearest, 11.8 against 17.4 ms with every term on
// (profiles/gridded_forcing.json).  No atomics, no LDS, no dependence between
// frames, nothing that depends on how the cells are cut into waves or shards:
// a frame's planes are the same bit for bit whichever call, batch position or
// shard produced them.
namespace tfg {

// One axis of a cell's stencil: the lower (or nearest) node, the step to the
// upper one (0 at a one-node axis and with nearest) and the weight of the
// upper node.
struct RegridAxis {
  int lo, step;
  double w;
};

// Model index k (global) on an axis of m nodes: coordinate o + s k.
// (Also evaluated on the host, for tfg_coarse_series's tables: the same fp64
// operations in the same order, without contraction.)
template <bool BIL>
__host__ __device__ __forceinline__ RegridAxis regrid_axis(double o, double s, int64_t k, int m) {
#pragma clang fp contract(off)
  const double t = o + s * (double)k;
  const double tc = fmin(fmax(t, 0.0), (double)(m - 1));
  RegridAxis a;
  if constexpr (BIL) {
    a.lo = min((int)floor(tc), max(m - 2, 0));
    a.step = min(a.lo + 1, m - 1) - a.lo;
    a.w = tc - (double)a.lo;
  } else {
    a.lo = (int)floor(tc + 0.5);
    a.step = 0;
    a.w = 0.0;
  }
  return a;
}

// A cell's stencil in a field [gny][gnx]: the byte offsets of its nodes
// (j0,i0), (j1,i0), (j0,i1), (j1,i1), or of the nearest node alone, and the
// weights.  A field is under 4 GiB (the entry point checks), so an offset is
// 32 bits and a gather is a buffer load: the field (frame, variable) as a
// wave-uniform descriptor in scalar registers plus one vector register.  With
// plain pointers the compiler keeps a 64-bit address per node, variable and
// lane across the frame loop (80 of them: 236 VGPRs, two waves per SIMD).
template <bool BIL>
struct RegridStencil {
  uint32_t o[BIL ? 4 : 1];
  double wy, wx;
};

template <bool BIL>
__device__ __forceinline__ RegridStencil<BIL> regrid_stencil(const RegridAxis& ya, const RegridAxis& xa, int gnx) {
  RegridStencil<BIL> st;
  const uint32_t row = (uint32_t)gnx * 8u, o00 = (uint32_t)ya.lo * row + (uint32_t)xa.lo * 8u;
  st.o[0] = o00;
  if constexpr (BIL) {
    st.o[1] = o00 + (uint32_t)ya.step * row;
    st.o[2] = o00 + (uint32_t)xa.step * 8u;
    st.o[3] = st.o[1] + (uint32_t)xa.step * 8u;
  }
  st.wy = ya.w;
  st.wx = xa.w;
  return st;
}

// A field of `bytes` bytes at a (wave-uniform) as a raw buffer: no stride, no
// swizzle, 32-bit data format; a load past `bytes` would return 0, not fault.
typedef __amdgpu_buffer_rsrc_t RegridField;
__device__ __forceinline__ RegridField regrid_field(const double* a, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ double regrid_node(RegridField a, uint32_t off) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(a, (int)off, 0, 0));
}

// A stencil's nodes of field a, and the value from them; apart, so that a
// caller can issue the loads of several stencils before the first lerp.
template <bool BIL>
struct RegridNodes {
  double a[BIL ? 4 : 1];
};

template <bool BIL>
__device__ __forceinline__ RegridNodes<BIL> regrid_gather(RegridField a, const RegridStencil<BIL>& st) {
  RegridNodes<BIL> nd;
#pragma unroll
  for (int k = 0; k < (BIL ? 4 : 1); ++k) nd.a[k] = regrid_node(a, st.o[k]);
  return nd;
}

template <bool BIL>
__device__ __forceinline__ double regrid_value(const RegridNodes<BIL>& nd, const RegridStencil<BIL>& st) {
#pragma clang fp contract(off)
  if constexpr (!BIL) {
    return nd.a[0];
  } else {
    const double west = nd.a[0] + st.wy * (nd.a[1] - nd.a[0]);
    const double east = nd.a[2] + st.wy * (nd.a[3] - nd.a[2]);
    return west + st.wx * (east - west);
  }
}

// tfg_set_inputs order (a source's fields) -> frame plane, as forcing_cell<false> maps them.
constexpr int kInputPlane[5] = {F_PA, F_Q, F_P, F_T, F_UZ};

// k_forcing_expand's store of one plane: a lane's V cells from q on, rounded
// already.  A lane whose V cells all lie under n (full) stores them at once,
// 16 bytes with V = 4 (float) or 2 (double); a ragged lane cell by cell.
template <class R, int V>
__device__ __forceinline__ void forcing_store(R* __restrict__ q, const R (&o)[V], bool full, int64_t i0, int64_t n) {
  typedef R vec __attribute__((ext_vector_type(V)));
  if (full) {
    vec x;
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = o[j];
    *reinterpret_cast<vec*>(q) = x;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < n) q[j] = o[j];
  }
}

}  // namespace tfg

// fr, nb, elev, n, n_pad: as k_forcing_expand's; src: [nb][5][gny][gnx] of the
// same frames; z_src [gny][gnx] is read only with DS; nx: cells per model row.
// A frame's 20 V gathers are independent.  Left alone the compiler issues them
// all at once (256 VGPRs, one wave per SIMD, nothing to overlap the stores
// with); told to keep more waves it issues them four at a time with a full
// wait after each.  So the frame is cut by scheduling barriers into groups
// whose loads are all issued before their first lerp: plain, a variable at a
// time (4 V loads, then its plane's store); with DS, which needs a cell's
// five values together, a cell at a time (20 loads).
template <class R, bool DS, bool BIL, int V>
__global__ __launch_bounds__(kBlock) void k_forcing_regrid(R* __restrict__ fr, int64_t n_pad, int nb,
                                                           const double* __restrict__ src,
                                                           const double* __restrict__ z_src,
                                                           const R* __restrict__ elev, int64_t n, int64_t nx,
                                                           tfg_forcing_grid g, ForcingDs d) {
  constexpr int kTile = kBlock * V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ntiles = (n + kTile - 1) / kTile;
  const int64_t t0 = (int64_t)blockIdx.x * ntiles / gridDim.x, t1 = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  const int64_t fstride = (int64_t)kNumForc * n_pad;
  const int64_t gnode = (int64_t)g.gny * g.gnx;
  const uint32_t fbytes = (uint32_t)gnode * 8u;  // a field, under 4 GiB
  const int loff = lane * V;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t wbase = t * kTile + wave * (64 * V);  // the wave's first cell: wave-uniform
    const int64_t i0 = wbase + loff;
    // once per cell and batch: the stencil, and with DS what hangs on dz alone
    tfg::RegridStencil<BIL> st[V];
    int xl[V], xs[V];       // a cell's lower (nearest) source column and the step to the upper one
    uint32_t yo0 = 0, yo1 = 0;  // the byte offsets of the first cell's two source rows
    double pfac[V], dT[V], xP[V];
    // row and column of the lane's first cell (cell n-1 past the end); the
    // next cells follow by stepping, one division per lane and tile
    const int64_t ic = i0 < n ? i0 : n - 1;
    int64_t r = (((uint64_t)ic | (uint64_t)nx) >> 32) == 0 ? (int64_t)((uint32_t)ic / (uint32_t)nx) : ic / nx;
    int64_t c = ic - r * nx;
    const int rfirst = (int)r;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (j > 0 && i0 + j < n && ++c == nx) {
        c = 0;
        ++r;
      }
      const tfg::RegridAxis ya = tfg::regrid_axis<BIL>(g.y0, g.sy, g.row0 + r, g.gny);
      const tfg::RegridAxis xa = tfg::regrid_axis<BIL>(g.x0, g.sx, c, g.gnx);
      st[j] = tfg::regrid_stencil<BIL>(ya, xa, g.gnx);
      xl[j] = xa.lo;
      xs[j] = xa.step;
      if (j == 0) {
        yo0 = (uint32_t)ya.lo * ((uint32_t)g.gnx * 8u);
        yo1 = yo0 + (uint32_t)ya.step * ((uint32_t)g.gnx * 8u);
      }
      if constexpr (DS) {
#pragma clang fp contract(off)
        const double dz = (double)elev[r * nx + c] - tfg::regrid_value<BIL>(tfg::regrid_gather<BIL>(tfg::regrid_field(z_src, fbytes), st[j]), st[j]);
        pfac[j] = fmax(0.0, 1.0 + d.grad_P * dz);
        dT[j] = d.lapse_T * dz;
        xP[j] = d.negM_g_R * dz;
      }
    }
    const bool full = i0 + V <= n;
    // The wave's cells run along the model grid, so rows and source columns are
    // monotonic over its lanes: lane 0's first and lane 63's last cell bound
    // both.  (The rows differ by less than 2^31, so their low words decide.)
    const bool one_row = __shfl(rfirst, 0) == __shfl((int)r, 63);
    const int ca = __shfl(xl[0], 0), cb = __shfl(xl[V - 1], 63);
    const int cmin = min(ca, cb), cmax = max(max(ca + __shfl(xs[0], 0), cb + __shfl(xs[V - 1], 63)), max(ca, cb));
    // In a wave that lies in one model row over at most 64 source columns (a
    // source coarser than the model) j0, j1 and wy are the wave's: lane L forms
    // the column value (the vertical lerp) of source column cmin + L once per
    // field, two loads, and a cell reads its west and east column from the
    // lanes that own them.  The same expression as a lane's own four gathers,
    // so the same bits.  Any other wave gathers per lane.
    const uint32_t oc = (uint32_t)min(cmin + lane, cmax) * 8u;
    auto column = [&](tfg::RegridField a) {
#pragma clang fp contract(off)
      const double lo = tfg::regrid_node(a, yo0 + oc);
      if constexpr (!BIL) return lo;
      else return lo + st[0].wy * (tfg::regrid_node(a, yo1 + oc) - lo);
    };
    auto pick = [&](double col, int j) {
#pragma clang fp contract(off)
      const double west = __shfl(col, xl[j] - cmin);
      if constexpr (!BIL) return west;
      else return west + st[j].wx * (__shfl(col, xl[j] + xs[j] - cmin) - west);
    };
    // The frames of the batch.  Plain, a field at a time: its gathers are all
    // issued before the first lerp, and its plane is stored at once.  With DS,
    // which needs a cell's five values together, a cell at a time.
    auto frames = [&](auto shared_tag) {
      constexpr bool SH = decltype(shared_tag)::value;
#pragma unroll 1
      for (int s = 0; s < nb; ++s) {
        const double* __restrict__ ss = src + (int64_t)s * 5 * gnode;
        R* const fp = fr + s * fstride + wbase + loff;  // plane 0 of the frame at the lane's first cell
        if constexpr (!DS) {
#pragma unroll
          for (int v = 0; v < 5; ++v) {
            const tfg::RegridField a = tfg::regrid_field(ss + v * gnode, fbytes);
            R o[V];  // rounded once
            if constexpr (SH) {
              const double col = column(a);
#pragma unroll
              for (int j = 0; j < V; ++j) o[j] = (R)pick(col, j);
            } else {
              tfg::RegridNodes<BIL> nd[V];
#pragma unroll
              for (int j = 0; j < V; ++j) nd[j] = tfg::regrid_gather<BIL>(a, st[j]);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < V; ++j) o[j] = (R)tfg::regrid_value<BIL>(nd[j], st[j]);
            }
            tfg::forcing_store<R, V>(fp + tfg::kInputPlane[v] * n_pad, o, full, i0, n);
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          double col[5];
          if constexpr (SH) {
#pragma unroll
            for (int v = 0; v < 5; ++v) col[v] = column(tfg::regrid_field(ss + v * gnode, fbytes));
            __builtin_amdgcn_sched_barrier(0);
          }
          R o[kNumForc][V];  // rounded once, as each cell is finished
#pragma unroll
          for (int j = 0; j < V; ++j) {
            double tv[5], x[kNumForc];
            if constexpr (SH) {
#pragma unroll
              for (int v = 0; v < 5; ++v) tv[v] = pick(col[v], j);
            } else {
              tfg::RegridNodes<BIL> nd[5];
#pragma unroll
              for (int v = 0; v < 5; ++v) nd[v] = tfg::regrid_gather<BIL>(tfg::regrid_field(ss + v * gnode, fbytes), st[j]);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int v = 0; v < 5; ++v) tv[v] = tfg::regrid_value<BIL>(nd[v], st[j]);
            }
            tfg::forcing_cell<true>(d, tv, pfac[j], dT[j], xP[j], x);
#pragma unroll
            for (int p = 0; p < kNumForc; ++p) o[p][j] = (R)x[p];
            __builtin_amdgcn_sched_barrier(0);  // one cell's arithmetic live at a time
          }
#pragma unroll
          for (int p = 0; p < kNumForc; ++p) tfg::forcing_store<R, V>(fp + p * n_pad, o[p], full, i0, n);
        }
      }
    };
    if (one_row && cmax - cmin < 64) frames(std::true_type{});
    else frames(std::false_type{});
  }
}
