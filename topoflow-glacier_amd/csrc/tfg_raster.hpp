// tfg_raster.hpp -- hydrofabric divides rasterised into the catchment-id
// raster on the device (gfx950): k_rasterize, a scanline polygon fill.
//
// Included by tfg_engine.hip after kBlock; the C ABI entry point
// (tfg_rasterize_polygons) lives there.
#pragma once

// ---------------------------------------------------------------------------
// The rule is hydrofabric.rasterize_divides' (numpy), restated: a cell's id is
// the id of the LAST polygon, in table order, whose shell contains the cell
// centre and none of whose holes does; a cell in no polygon gets outside_id.
// Containment is the even-odd crossing test: an edge (a, b) -> (c, d), b != d,
// crosses the row of centre ordinate py when (b > py) != (d > py), at
//   xc = a + (py - b) * (c - a) / (d - b),
// and counts for the cell of centre abscissa px when px < xc.  A polygon only
// writes cells of its host-computed half-open cell box (r0, r1, c0, c1), as
// numpy only visits those; outside it the parity is even anyway.
//
// Bitwise identity with numpy: the centres px [nx] and py [ny] come from the
// host, formed there by rasterize_divides' own expressions (hipcc would
// contract x0 + (col + 0.5) * cell into an FMA, numpy does not), and xc is
// formed in raster_xc with contraction off: four separately rounded fp64
// operations in numpy's order (the division is the compiler's correctly
// rounded fp64 sequence).  Everything else is comparisons and integers.
//
// Shape: xc depends on the edge and the row only, so a workgroup owns one row
// and one tile of kBlock * 4 columns, forms each crossing once and shares it
// through LDS; numpy recomputes it per edge and cell.  A lane holds 4
// consecutive cells.  The workgroup walks the polygons whose box holds its row
// and overlaps its tile (a workgroup-uniform test on four integers).  Per ring,
// in fills of kBlock edges (one edge per lane): a lane whose edge straddles the
// row computes xc; each wave packs its crossings into its own segment of the
// LDS list by ballot and prefix count (no atomics, a fixed order); after one
// barrier every lane counts px < xc over the four segments for its 4 cells.
// A fill holds at most kBlock crossings by construction, so a row with more
// crossings than that simply takes several fills, whose parities XOR: the
// result does not depend on the list's capacity.  The list is double-buffered
// by fill parity, which is what makes one barrier per fill enough (a fill's
// writers come after the barrier that the readers of the fill before last
// have passed).  Shell and holes combine per cell in registers
// (shell & ~hole & ...), later polygons overwrite earlier ids in registers,
// and the id plane is written once: one 16-byte store per lane when nx is a
// multiple of 4 (every row then starts 16-byte aligned), else per cell.  No
// cell at or past n = ny * nx is touched: the plane's padding stays as it is.
//
// Per-catchment cell counts (optional): integer atomics only, which are exact
// whatever their order: per wave a ballot per distinct id, one LDS add per
// wave and id, one global 64-bit add per workgroup and id present.
constexpr int kRasterCells = 4;                     // cells per lane
constexpr int kRasterTile = kBlock * kRasterCells;  // columns per workgroup
constexpr int kRasterMaxCatch = 512;                // tfg_create's bound on n_catch

// The device-side tables of one call (tfg_polygons, on the device).
struct RasterTables {
  const int32_t* poly_id;     // [n_poly]
  const int32_t* poly_ring0;  // [n_poly + 1]
  const int4* poly_box;       // [n_poly] r0, r1, c0, c1
  const int64_t* ring_edge0;  // [n_rings + 1]
  const double2* edges;       // [n_edges][2]: (a, b), (c, d)
  const double* px;           // [nx]
  const double* py;           // [ny]
  int32_t n_poly;
};

namespace tfg {

// numpy's a + (py - b) * (c - a) / (d - b): left to right, each operation rounded once
__device__ __forceinline__ double raster_xc(double a, double b, double c, double d, double py) {
#pragma clang fp contract(off)
  const double t = (py - b) * (c - a);
  const double q = t / (d - b);
  return a + q;
}

}  // namespace tfg

// ids: [ny * nx] of the handle's plane; cells: [n_catch] int64 counts, added to (zeroed by the caller), or null.
// Launched with ny * tiles workgroups, tiles = ceil(nx / kRasterTile).
__global__ __launch_bounds__(kBlock) void k_rasterize(int32_t* __restrict__ ids, int32_t ny, int32_t nx, int32_t tiles,
                                                      RasterTables t, int32_t outside_id, int32_t n_catch,
                                                      unsigned long long* __restrict__ cells) {
  constexpr int kWavesWg = kBlock / 64;
  __shared__ double s_xc[2][kWavesWg][64];
  __shared__ int32_t s_cnt[2][kWavesWg];
  __shared__ int32_t s_bins[kRasterMaxCatch];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t row = (int32_t)(blockIdx.x / (uint32_t)tiles), tile = (int32_t)(blockIdx.x % (uint32_t)tiles);
  const int32_t tc0 = tile * kRasterTile, tc1 = min(tc0 + kRasterTile, nx);  // the tile's columns
  const int32_t col0 = tc0 + tid * kRasterCells;
  const double py = t.py[row];
  double px[kRasterCells];
  int32_t id[kRasterCells];
#pragma unroll
  for (int j = 0; j < kRasterCells; ++j) {
    px[j] = t.px[min(col0 + j, nx - 1)];  // past the row's end: an in-bounds address, never stored
    id[j] = outside_id;
  }
  if (cells)
    for (int c = tid; c < n_catch; c += kBlock) s_bins[c] = 0;

  int buf = 0;  // the fill's half of the list
  for (int32_t p = 0; p < t.n_poly; ++p) {
    const int4 box = t.poly_box[p];
    if (row < box.x || row >= box.y || box.w <= tc0 || box.z >= tc1) continue;  // workgroup-uniform
    unsigned inside = 0;  // bit j: cell j is in the shell and in no hole so far
    const int32_t k0 = t.poly_ring0[p], k1 = t.poly_ring0[p + 1];
    for (int32_t k = k0; k < k1; ++k) {
      unsigned par = 0;  // bit j: crossings right of cell j, mod 2
      const int64_t e0 = t.ring_edge0[k], e1 = t.ring_edge0[k + 1];
      for (int64_t base = e0; base < e1; base += kBlock, buf ^= 1) {
        const int64_t e = base + tid;
        bool cross = false;
        double xc = 0.0;
        if (e < e1) {
          const double2 ab = t.edges[2 * e], cd = t.edges[2 * e + 1];
          cross = (ab.y > py) != (cd.y > py);
          if (cross) xc = tfg::raster_xc(ab.x, ab.y, cd.x, cd.y, py);
        }
        const unsigned long long m = __ballot(cross);
        if (cross) s_xc[buf][wave][__popcll(m & ((1ull << lane) - 1))] = xc;
        if (lane == 0) s_cnt[buf][wave] = __popcll(m);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWavesWg; ++w) {
          const int nc = s_cnt[buf][w];
          for (int i = 0; i < nc; ++i) {
            const double x = s_xc[buf][w][i];  // one address per wave: a broadcast read
#pragma unroll
            for (int j = 0; j < kRasterCells; ++j) par ^= (unsigned)(px[j] < x) << j;
          }
        }
      }
      inside = k == k0 ? par : inside & ~par;
    }
    const int32_t pid = t.poly_id[p];
#pragma unroll
    for (int j = 0; j < kRasterCells; ++j) {
      const int32_t c = col0 + j;
      if (((inside >> j) & 1u) && c >= box.z && c < box.w) id[j] = pid;
    }
  }

  const int64_t at = (int64_t)row * nx + col0;
  if (col0 < nx) {
    if ((nx & 3) == 0) {  // col0 + 4 <= nx, and the row starts 16-byte aligned
      *reinterpret_cast<int4*>(ids + at) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kRasterCells; ++j)
        if (col0 + j < nx) ids[at + j] = id[j];
    }
  }

  if (cells) {  // workgroup-uniform
    __syncthreads();  // the bins are zeroed
#pragma unroll
    for (int j = 0; j < kRasterCells; ++j) {
      bool todo = col0 + j < nx;
      while (__any(todo)) {
        // the first pending lane's id, counted for every lane that shares it
        const int32_t c = __shfl(id[j], __ffsll((long long)__ballot(todo)) - 1);
        const bool mine = todo && id[j] == c;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) atomicAdd(&s_bins[c], (int32_t)__popcll(m));
        todo = todo && !mine;
      }
    }
    __syncthreads();
    for (int c = tid; c < n_catch; c += kBlock)
      if (s_bins[c]) atomicAdd(cells + c, (unsigned long long)s_bins[c]);
  }
}
