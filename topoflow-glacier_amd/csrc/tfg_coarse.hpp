// tfg_coarse.hpp -- per-node sums and counts of history planes on a regular
// coarse grid, device side (gfx950).
//
// Included by tfg_engine.hip after tfg_series.hpp (kSeriesBatch) and
// tfg_forcing.hpp (tfg::regrid_axis); the C ABI entry point (tfg_coarse_series)
// lives in tfg_engine.hip.
#pragma once

// ---------------------------------------------------------------------------
// Coarse series (tfg_coarse_series): for one history field, a batch of
// kCoarseBatch history slots and the nodes (J, I) of a tfg_forcing_grid,
//   sum  [slot][J][I] = sum over the cells (r, c) of node (J, I) of
//                       hist[slot][field][r nx + c]                          fp64
//   count[slot][J][I] = number of those cells with (double)value > threshold
//   cells      [J][I] = number of cells of node (J, I) = rows(J) cols(I)
// The adjoint of nearest-neighbour gridded forcing: a cell belongs to the node
// whose forcing it receives, J = regrid_axis<false>(y0, sy, row0 + r, gny).lo,
// I alike from c.  What a coupled run hands back to the atmospheric model per
// step, and the only way to write step-wise maps of a large run without the
// planes leaving the device.
//
// Key.  J depends on the row alone and I on the column alone, and both maps
// are monotone, so a node owns a rectangle of cells: there is no id raster, no
// ballot loop, no bin per key and no atomic.  The host evaluates
// tfg::regrid_axis<false> -- the function k_forcing_regrid evaluates, in fp64
// without contraction -- once per row and per column of a grid (ny + nx
// evaluations) and derives the tables below (coarse_plan); they are cached on
// the handle against the grid struct's bytes and uploaded through the pinned
// staging ring, so a call with the grid of the call before queues kernels only.
//   segments  every run of model rows that share a J, cut into pieces of at
//             most kCoarseSegRows rows: a source of a few nodes, or of one,
//             still fills the chip.  The segments tile [0, ny).
//   pairs     every run of model columns that share an I, cut at the multiples
//             of 64 V columns (V = 16 / sizeof(R) columns per lane: what a wave
//             covers).  A pair lies in one wave of one tile, and a node's pairs
//             are consecutive.  pcol[c] is column c's pair, P their number.
//
// Shape (k_coarse_series).  A workgroup takes one segment x one tile of
// kBlock V columns; a lane keeps V consecutive columns x kCoarseBatch slots of
// fp64 accumulators and walks the segment's rows in ascending order.  Per row
// a lane issues one 16-byte load per slot (VEC: nx a multiple of V, so every
// row is 16-byte aligned and a lane's V columns lie on one side of the row
// end) or V scalar loads per slot (any nx), all of them before the first is
// used, and the next row's before the current row is added (the last trip
// loads its own row again: no branch around the loads).  Columns at or past
// the row end load an in-bounds address of the same row and contribute a
// selected 0; a wave whose columns all lie past the row end leaves at once
// (the workgroup has no barrier).  Each plane element is read once per call;
// the address and key work of a row serves the batch's slots.
// Counts are kept per column in 32 / V-bit fields of one register per slot
// (a segment has at most kCoarseSegRows < 2^8 rows).
//
// At the segment's end a wave reduces its columns to its pairs in registers:
// a lane scans its V columns (a run of equal pairs is summed left to right),
// the lanes' trailing runs go through a segmented inclusive scan over the
// lanes (__shfl_up by 1, 2, 4, 8, 16, 32; a lane whose columns are one pair
// that continues the lane before it passes the sum on, any other lane starts
// a segment), and the lane holding a pair's last column adds what the lanes
// before it carry and stores the pair: part_sum[segment][slot][pair] fp64,
// part_cnt likewise int32.  No LDS, no barrier.  Which lanes add at which
// step is a function of pcol alone, the same for every slot: a select, never
// a product, so a NaN reaches the pair of its own column in its own slot and
// nothing else.
//
// Fold (k_coarse_fold), output driven: one thread (or TH = 16 or 256 threads,
// by the longest list of any node: coarse_plan) per (slot, node) adds the
// node's partials in (segment, pair) order -- TH threads take every TH-th term
// in that order and meet in a fixed LDS tree -- and stores the entry: a node
// without cells has no term and reads 0.  cells needs no plane and no partial:
// k_coarse_cells writes rows(J) cols(I).
//
// No floating-point atomics, no dependence on dispatch order or on the
// device's CU count: segments, pairs, the scan's steps and TH follow from the
// grid geometry and compile-time constants alone, so two calls give the same
// bits, and a (slot, node) entry does not depend on which other slots share
// the call, where in a batch it sits (a short last batch loads its last slot
// again in the unused positions and stores nothing for them) or where the
// output lives.
//
// What a call needs of the handle (the tables a cache of their own, the rest
// the history readers' shared scratch), none of it depending on nslots:
//   tables    (nx + nseg + 1 + 3 gny + 3 gnx) * 4 B
//   partials  kCoarseBatch * nseg * P * (8 + 4) B, with
//             nseg <= min(ny, gny + ny / kCoarseSegRows) and
//             P    <= min(nx, gnx + nx / (64 V)):
//             8192^2 fp32 cells under 257^2 nodes: 512 * 288 * 96 B = 14.2 MB;
//             never more than 96 B per cell of the shard (a source as fine as
//             the model, whose own output is 8 B per cell and slot)
//   a host-output call's device copy of one batch: kCoarseBatch * gny * gnx *
//             16 B and gny * gnx * 8 B of cells; the call copies each batch out.
//
// Longest chain of dependent fp64 additions of one entry: kCoarseSegRows - 1
// (a column) + V - 1 + 6 + 1 (the wave) + terms / TH + log2(TH) (the fold).
//
// Measured (tests/diagnostics/coarse_series_timing.py, profiles/coarse_series.json;
// fp32 engine, one 24-slot M_total call, device events, medians of 10): at
// 8192^2 under 257^2 nodes the sums-only call takes 1.08 ms, 5.96 TB/s on the
// 6.44 GB it must read, against 1.58 ms (4.57 TB/s on 7.25 GB) for the same
// slots' tfg_catchment_series in the same process: 0.68 of it; with counts
// 1.12 ms; 33^2 nodes 1.06 ms, one node 1.15 ms; cells alone 0.01 ms.  The
// segment length hardly matters between 8 and 64 rows (1.10, 1.08, 1.12 and
// 1.12 ms at 8, 16, 32 and 64 rows under 257^2 nodes; 1.26, 1.15, 1.15 and
// 1.14 ms under one node).  k_coarse_series runs at 140 VGPRs (159 with
// counts), three waves per SIMD; asking for four (128 VGPRs) costs half as
// much again (1.65 ms).
#ifndef TFG_COARSE_SEG_ROWS  // diagnostic builds time other lengths (tests/diagnostics/coarse_series_timing.py)
#define TFG_COARSE_SEG_ROWS 16
#endif
constexpr int kCoarseBatch = kSeriesBatch;            // history slots per launch
constexpr int kCoarseSegRows = TFG_COARSE_SEG_ROWS;  // rows of a segment, at most
static_assert(kCoarseSegRows < 256, "a column's count lives in an 8-bit field");

// Offsets (in int32 elements) of the tables in the handle's device copy, and
// what the launches need of the plan.
struct CoarsePlan {
  int nseg = 0, P = 0, ntiles = 0, fold_th = 1;
  size_t o_pcol = 0, o_seg = 0, o_segj = 0, o_pairi = 0, o_rows = 0, o_cols = 0, len = 0;
};

// The tables of grid g over a shard of ny x nx cells with v columns per lane:
//   pcol  [nx]        the pair of column c
//   seg   [nseg + 1]  the first row of segment s; seg[nseg] = ny
//   segj  [gny][2]    node row J's segments [first, end)
//   pairi [gnx][2]    node column I's pairs [first, end)
//   rows  [gny], cols [gnx]   model rows of J, model columns of I
inline CoarsePlan coarse_plan(int64_t ny, int64_t nx, const tfg_forcing_grid& g, int v, std::vector<int32_t>& tab) {
  CoarsePlan p;
  const size_t gny = (size_t)g.gny, gnx = (size_t)g.gnx;
  std::vector<int32_t> seg;
  std::vector<int32_t> segj(2 * gny, 0), pairi(2 * gnx, 0), rows(gny, 0), cols(gnx, 0), pcol((size_t)nx);
  int jprev = -1, run = 0;
  for (int64_t r = 0; r < ny; ++r) {
    const int j = tfg::regrid_axis<false>(g.y0, g.sy, g.row0 + r, g.gny).lo;
    if (r == 0 || j != jprev || run == kCoarseSegRows) {
      if (r == 0 || j != jprev) segj[2 * (size_t)j] = (int32_t)seg.size();
      seg.push_back((int32_t)r);
      run = 0;
    }
    ++run;
    ++rows[j];
    segj[2 * (size_t)j + 1] = (int32_t)seg.size();
    jprev = j;
  }
  p.nseg = (int)seg.size();
  seg.push_back((int32_t)ny);
  const int64_t wcols = 64 * (int64_t)v;
  int iprev = -1, np = 0;
  for (int64_t c = 0; c < nx; ++c) {
    const int i = tfg::regrid_axis<false>(g.x0, g.sx, c, g.gnx).lo;
    if (c == 0 || i != iprev || c % wcols == 0) {
      if (c == 0 || i != iprev) pairi[2 * (size_t)i] = np;
      ++np;
    }
    pcol[(size_t)c] = np - 1;
    ++cols[i];
    pairi[2 * (size_t)i + 1] = np;
    iprev = i;
  }
  p.P = np;
  p.ntiles = (int)((nx + kBlock * wcols / 64 - 1) / (kBlock * wcols / 64));
  int64_t max_seg = 0, max_pair = 0;
  for (size_t j = 0; j < gny; ++j) max_seg = std::max<int64_t>(max_seg, segj[2 * j + 1] - segj[2 * j]);
  for (size_t i = 0; i < gnx; ++i) max_pair = std::max<int64_t>(max_pair, pairi[2 * i + 1] - pairi[2 * i]);
  const int64_t terms = max_seg * max_pair;  // the longest list a fold thread group adds
  p.fold_th = terms <= 8 ? 1 : terms <= 512 ? 16 : 256;
  tab.clear();
  auto put = [&](const std::vector<int32_t>& a) {
    const size_t at = tab.size();
    tab.insert(tab.end(), a.begin(), a.end());
    return at;
  };
  p.o_pcol = put(pcol);
  p.o_seg = put(seg);
  p.o_segj = put(segj);
  p.o_pairi = put(pairi);
  p.o_rows = put(rows);
  p.o_cols = put(cols);
  p.len = tab.size();
  return p;
}

// plane, slot_stride, hist_depth, slot0, nb: as k_catch_series (position s
// reads slot (slot0 + min(s, nb - 1)) % hist_depth).  seg, pcol: coarse_plan's
// tables; blockIdx.x = segment * ntiles + tile.  part_sum, part_cnt:
// [nseg][kCoarseBatch][P].  VEC: nx is a multiple of V and the planes are
// 16-byte aligned.
template <class R, bool VEC, bool SUM, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_coarse_series(const R* __restrict__ plane, int64_t slot_stride, int hist_depth,
                                                          int slot0, int nb, int nx, const int32_t* __restrict__ seg,
                                                          const int32_t* __restrict__ pcol, int ntiles, int P, double thr,
                                                          double* __restrict__ part_sum, int32_t* __restrict__ part_cnt) {
  constexpr int NB = kCoarseBatch;
  constexpr int V = 16 / (int)sizeof(R);  // columns per lane
  constexpr int kField = 32 / V;          // bits of a column's count
  typedef R vec __attribute__((ext_vector_type(V)));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sg = blockIdx.x / ntiles, tile = blockIdx.x - sg * ntiles;
  const int wc0 = (tile * kWaves + wave) * (64 * V);  // the wave's first column
  if (wc0 >= nx) return;                              // wave-uniform: no column of this wave is in the row
  const int c0 = wc0 + lane * V;
  const int r0 = seg[sg], r1 = seg[sg + 1];

  // once per workgroup: a column's pair (-1 past the row end) and the column it loads
  int q[V], cl[V];
  bool in[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    in[j] = c0 + j < nx;
    cl[j] = VEC ? (in[0] ? c0 : nx - V) + j : min(c0 + j, nx - 1);
    q[j] = in[j] ? pcol[cl[j]] : -1;
  }

  const R* sp[NB];
#pragma unroll
  for (int s = 0; s < NB; ++s) sp[s] = plane + (int64_t)((slot0 + (s < nb ? s : nb - 1)) % hist_depth) * slot_stride;

  // a row's loads: the lane's V columns in every position (a shard is under 2^29 cells)
  auto load = [&](int r, R (&x)[NB][V]) {
    const uint32_t row = (uint32_t)r * (uint32_t)nx;
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      if constexpr (VEC) {
        const vec t = *reinterpret_cast<const vec*>(sp[s] + (row + (uint32_t)cl[0]));
#pragma unroll
        for (int j = 0; j < V; ++j) x[s][j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[s][j] = sp[s][row + (uint32_t)cl[j]];
      }
    }
  };

  double acc[NB][V] = {};
  uint32_t cnt[NB] = {};
  R x[NB][V];
  load(r0, x);
  for (int r = r0; r < r1; ++r) {
    // the next row's loads are in flight while this one is added (the last trip
    // loads its own row again: no branch around the loads)
    R x_n[NB][V];
    load(r + 1 < r1 ? r + 1 : r, x_n);
#pragma unroll
    for (int s = 0; s < NB; ++s) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double v = (double)x[s][j];
        if constexpr (SUM) acc[s][j] += in[j] ? v : 0.0;
        if constexpr (COUNT) cnt[s] += (in[j] && v > thr) ? 1u << (kField * j) : 0u;
      }
    }
#pragma unroll
    for (int s = 0; s < NB; ++s)
#pragma unroll
      for (int j = 0; j < V; ++j) x[s][j] = x_n[s][j];
  }

  // The wave's columns to its pairs.  What does not depend on the slot: where a
  // pair ends, whether the lane before carries into this one, and the lanes
  // that add at each step of the scan over the lanes' trailing runs.
  const int q_up = __shfl_down(q[0], 1), q_down = __shfl_up(q[V - 1], 1);
  bool end[V];
#pragma unroll
  for (int j = 0; j < V; ++j) end[j] = in[j] && (j + 1 < V ? q[j + 1] != q[j] : (lane == 63 || q_up != q[j]));
  const bool cont = lane > 0 && q_down == q[0];  // the pair of the first column began in a lane before
  bool head = !(cont && q[0] == q[V - 1]);       // any lane but one that only passes a pair on
  uint32_t adds = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int h_down = __shfl_up((int)head, 1 << i);  // every lane takes part
    if (lane >= (1 << i)) {
      adds |= head ? 0u : 1u << i;
      head = head || h_down;
    }
  }
  // a pair's total from the lane's scan r[] of its columns and the lanes' scan t of their trailing runs
  auto wave_pairs = [&](auto zero, auto&& column, auto&& store) {
    using T = decltype(zero);
    T r[V];
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = (j > 0 && q[j] == q[j - 1]) ? r[j > 0 ? j - 1 : 0] + column(j) : column(j);
    T t = r[V - 1];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const T t_down = __shfl_up(t, 1 << i);
      t = ((adds >> i) & 1u) ? t_down + t : t;
    }
    const T carry = __shfl_up(t, 1);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (end[j]) store(q[j], (cont && q[j] == q[0]) ? carry + r[j] : r[j]);
  };
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    const int64_t row = ((int64_t)sg * NB + s) * P;
    const bool used = s < nb;
    if constexpr (SUM)
      wave_pairs(0.0, [&](int j) { return acc[s][j]; }, [&](int pair, double v) { if (used) part_sum[row + pair] = v; });
    if constexpr (COUNT)
      wave_pairs(0, [&](int j) { return (int)((cnt[s] >> (kField * j)) & ((1u << kField) - 1u)); },
                 [&](int pair, int v) { if (used) part_cnt[row + pair] = v; });
  }
}

// out[s][J][I] = the sum of part[segment][s][pair] over node row J's segments
// and node column I's pairs in (segment, pair) order, s < nb.  TH threads per
// entry (kBlock / TH entries per workgroup, consecutive threads on consecutive
// entries): thread k of an entry adds the terms k, k + TH, ... in order, and
// the TH sums meet pairwise over LDS (k_series_reduce's tree).
template <class T, class O, int TH>
__global__ __launch_bounds__(kBlock) void k_coarse_fold(const T* __restrict__ part, int nb, int gny, int gnx, int P,
                                                        const int32_t* __restrict__ segj, const int32_t* __restrict__ pairi,
                                                        O* __restrict__ out) {
  constexpr int kEntries = kBlock / TH;
  const int x = threadIdx.x % kEntries, k = threadIdx.x / kEntries;
  const int64_t nodes = (int64_t)gny * gnx, nent = (int64_t)nb * nodes;
  const int64_t e = (int64_t)blockIdx.x * kEntries + x;
  O v = 0;
  if (e < nent) {
    const int s = (int)(e / nodes);
    const int64_t node = e - s * nodes;
    const int J = (int)(node / gnx), I = (int)(node - (int64_t)J * gnx);
    const int s0 = segj[2 * J], s1 = segj[2 * J + 1], p0 = pairi[2 * I], p1 = pairi[2 * I + 1];
    if constexpr (TH == 1) {
      for (int sg = s0; sg < s1; ++sg) {
        const T* row = part + ((int64_t)sg * kCoarseBatch + s) * P;
        for (int p = p0; p < p1; ++p) v += (O)row[p];
      }
    } else {
      const int np = p1 - p0;
      const int64_t terms = (int64_t)(s1 - s0) * np;
      for (int64_t t = k; t < terms; t += TH) {
        const int ds = (int)(t / np);
        v += (O)part[((int64_t)(s0 + ds) * kCoarseBatch + s) * P + p0 + (int)(t - (int64_t)ds * np)];
      }
    }
  }
  if constexpr (TH == 1) {
    if (e < nent) out[e] = v;
  } else {
    __shared__ O red[TH][kEntries + 1];
    red[k][x] = v;
    __syncthreads();
    for (int h = TH / 2; h > 0; h >>= 1) {
      if (k < h) red[k][x] += red[k + h][x];
      __syncthreads();
    }
    if (k == 0 && e < nent) out[e] = red[0][x];
  }
}

// cells[J][I] = rows(J) cols(I)
__global__ __launch_bounds__(kBlock) void k_coarse_cells(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                         int gny, int gnx, int64_t* __restrict__ cells) {
  const int64_t nodes = (int64_t)gny * gnx;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nodes; i += (int64_t)gridDim.x * kBlock) {
    const int J = (int)(i / gnx);
    cells[i] = (int64_t)rows[J] * cols[i - (int64_t)J * gnx];
  }
}
