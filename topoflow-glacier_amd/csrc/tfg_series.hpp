// tfg_series.hpp -- per-catchment sums of history planes, device side (gfx950).
//
// Included by tfg_engine.hip after the history layout (kNumHist, H_*) and
// kBlock / kWaves; the C ABI entry point (tfg_catchment_series) lives there.
#pragma once

// ---------------------------------------------------------------------------
// Catchment series (tfg_catchment_series): for one history field and a batch
// of up to kSeriesBatch history slots,
//   sum[slot][c] = sum over cells i < n with catch_id[i] == c of
//                  hist[slot][field][i],                      fp64 throughout.
// What a caller of the reference gets from M_total * da_m2 of one catchment
// per step (examples/run_topoflow_glacier.py:112), for every catchment of a
// raster and every step still in the history, without the planes leaving the
// device.
//
// Shape: k_fused's diagnostic reduction.  Workgroups own whole, aligned chunks
// of kBlock cells (the same partition of the chunks over the grid).  Per chunk
// a lane loads its cell's id once and the cell's value in every slot of the
// batch, all of them before the first is used: with eight slots a wave has
// nine loads in flight, eighteen with the next chunk's.  Cells at or past n
// (a ragged last chunk, the plane padding) are excluded by index: they load
// cell n-1 (an in-bounds address, no branch around a load) and contribute a
// selected 0.  Per wave and per
// distinct id in the wave (wave_flush's ballot / leader loop: one pass when
// the wave holds one id, the normal case on a real divide raster) the values
// go through a fixed __shfl_xor butterfly (series_wave_sums: the eight
// positions in ten exchanges), and eight lanes add the wave's sums to LDS bins
// [kSeriesBatch][n_catch] that the four waves share, taking turns in wave
// order: 64 B per catchment, 32 KiB at tfg_create's limit of 512 (per-wave
// bins would be 128 KiB).  A wave with one id forms its sums before its turn,
// and the next chunk's loads are issued before the current chunk is reduced.
// A workgroup ends by storing its bins as one row of partials, which
// k_series_reduce folds over the workgroups in a fixed order.
//
// No floating-point atomics, no dependence on dispatch order: a call's result
// is bit-reproducible.  Every slot goes through the same operations on its
// own values alone -- the slots of a batch share only the ids and the control
// flow -- and the workgroup count depends on the grid and n_catch only, so a
// slot's row does not depend on which other slots share the call or where in
// a batch it sits.  A short last batch loads its last slot again in the unused
// positions (the same addresses: cache hits) and stores no row for them.  A
// NaN reaches exactly the (slot, catchment) entry of its cell: other ids'
// passes and other slots see a selected 0, never a product.
//
// Scratch: partials [workgroups][kSeriesBatch][n_catch] fp64, in the scratch
// the history readers share.  series_blocks() caps the workgroups at
// kSeriesMaxBlocks and at kSeriesScratchMax / (kSeriesBatch * n_catch * 8), and
// a call loops over batches of kSeriesBatch slots, so the scratch stays at or
// under 64 MiB whatever the arguments: 4096 rows of 64 B * n_catch up to 256
// catchments, 2048 rows of 32 KiB (64 MiB) at 512.
//
// Longest chain of dependent fp64 additions of one entry: 6 (butterfly) +
// 4 * chunks per workgroup (the bins) + workgroups / 16 + 4 (the fold).  At
// 8192^2 cells (262144 chunks): 6 + 256 + 256 + 4 = 522 up to 256 catchments,
// 6 + 512 + 128 + 4 = 650 at 512.
constexpr int kSeriesBatch = 8;                         // history slots per launch
constexpr int kSeriesMaxBlocks = 4096;                  // 16 workgroups per CU
constexpr int64_t kSeriesScratchMax = (int64_t)64 << 20;  // bytes of partials

// Workgroups of a k_catch_series launch over n cells (= rows of partials).
inline int series_blocks(int64_t n, int n_catch) {
  const int64_t chunks = (n + kBlock - 1) / kBlock;
  const int64_t by_scratch = kSeriesScratchMax / ((int64_t)kSeriesBatch * n_catch * 8);
  return (int)std::max<int64_t>(1, std::min<int64_t>({chunks, (int64_t)kSeriesMaxBlocks, by_scratch}));
}

// The sums of a wave's eight values per lane (v[s]: position s of the batch),
// by a butterfly that halves the values a lane carries at each of its first
// three levels: at xor 32 a lane keeps positions 0-3 (lanes 0-31) or 4-7
// (lanes 32-63) and sends the other four, at 16 it keeps two of its four, at 8
// one of its two; levels 4, 2 and 1 then sum that one.  Ten exchanges where
// eight plain butterflies take 48, and for every position the same pairs in
// the same order, xor 32, 16, 8, 4, 2, 1 (which lane of a pair adds does not
// matter: a + b = b + a), so a position's sum does not depend on the position.
// Returns, in every lane, the wave's sum of position lane >> 3.
static_assert(kSeriesBatch == 8, "series_wave_sums folds eight positions over the lane bits 5, 4, 3");
__device__ __forceinline__ double series_wave_sums(const double (&v)[kSeriesBatch], int lane) {
  double a[4], b[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (h5 ? v[4 + j] : v[j]) + __shfl_xor(h5 ? v[j] : v[4 + j], 32);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = (h4 ? a[2 + j] : a[j]) + __shfl_xor(h4 ? a[j] : a[2 + j], 16);
  double t = (h3 ? b[1] : b[0]) + __shfl_xor(h3 ? b[0] : b[1], 8);
  t += __shfl_xor(t, 4);
  t += __shfl_xor(t, 2);
  t += __shfl_xor(t, 1);
  return t;
}

// plane: the field's plane of history slot 0 (hist + field_index * n_pad);
// slot_stride = kNumHist * n_pad elements.  Position s of the batch reads slot
// (slot0 + min(s, nb - 1)) % hist_depth.  part: [gridDim.x][kSeriesBatch][n_catch].
// CATCH: an id raster is set (k_fused's CATCH); without one every cell is in
// catchment 0, and no load hangs on a run-time pointer test.
template <class R, bool CATCH>
__global__ __launch_bounds__(kBlock) void k_catch_series(const R* __restrict__ plane, int64_t slot_stride, int hist_depth,
                                                         int slot0, int nb,
                                                         const int32_t* __restrict__ catch_id,  // [n_pad] (CATCH)
                                                         int64_t n, int n_catch, double* __restrict__ part) {
  extern __shared__ double series_bins[];  // [kSeriesBatch][n_catch]
  const int nbins = kSeriesBatch * n_catch;
  for (int i = threadIdx.x; i < nbins; i += kBlock) series_bins[i] = 0.0;
  __syncthreads();

  const R* sp[kSeriesBatch];
#pragma unroll
  for (int s = 0; s < kSeriesBatch; ++s)
    sp[s] = plane + (int64_t)((slot0 + (s < nb ? s : nb - 1)) % hist_depth) * slot_stride;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nchunks = (n + kBlock - 1) / kBlock;
  const int64_t wg = blockIdx.x;
  const int64_t c0 = wg * nchunks / gridDim.x, c1 = (wg + 1) * nchunks / gridDim.x;
  double* const mybin = series_bins + (lane >> 3) * n_catch;  // the position this lane holds after series_wave_sums
  const bool writer = (lane & 7) == 0;

  // a chunk's loads: the id once per cell, then the cell in every position
  auto load = [&](int64_t ch, int& cid, R (&x)[kSeriesBatch]) {
    const int64_t i = ch * kBlock + threadIdx.x;
    const int64_t il = i < n ? i : n - 1;
    if constexpr (CATCH) cid = catch_id[il]; else cid = 0;
#pragma unroll
    for (int s = 0; s < kSeriesBatch; ++s) x[s] = sp[s][il];
  };
  int cid = 0;
  R x[kSeriesBatch] = {};
  if (c0 < c1) load(c0, cid, x);
  for (int64_t ch = c0; ch < c1; ++ch) {
    // the next chunk's loads are in flight while this one is reduced (the last
    // trip loads its own chunk again: no branch around the loads)
    int cid_n;
    R x_n[kSeriesBatch];
    load(ch + 1 < c1 ? ch + 1 : ch, cid_n, x_n);
    const bool has = ch * kBlock + threadIdx.x < n;
    const uint64_t active = __ballot(has);
    const int c_first = __shfl(cid, active ? __builtin_ctzll(active) : 0);
    // the normal case on a real divide raster: one id in the wave.  Its sums
    // are formed before the wave's turn, which is then one LDS add per position
    const bool one_id = __ballot(has && cid == c_first) == active;
    double t = 0.0;
    if (one_id) {
      double v[kSeriesBatch];
#pragma unroll
      for (int s = 0; s < kSeriesBatch; ++s) v[s] = has ? (double)x[s] : 0.0;
      t = series_wave_sums(v, lane);
    }
    for (int turn = 0; turn < kWaves; ++turn) {
      if (wave == turn) {
        if (one_id) {
          if (active && writer) mybin[c_first] += t;
        } else {
          uint64_t pending = active;
          while (pending) {  // a pass per distinct id of the wave (wave_flush's loop)
            const int c = __shfl(cid, __builtin_ctzll(pending));
            const bool mine = has && (cid == c);
            double v[kSeriesBatch];
#pragma unroll
            for (int s = 0; s < kSeriesBatch; ++s) v[s] = mine ? (double)x[s] : 0.0;
            const double tc = series_wave_sums(v, lane);
            if (writer) mybin[c] += tc;
            pending &= ~__ballot(mine);
          }
        }
      }
      __syncthreads();
    }
    cid = cid_n;
#pragma unroll
    for (int s = 0; s < kSeriesBatch; ++s) x[s] = x_n[s];
  }
  // the last turn's barrier (or the one after the zeroing) made the bins visible
  double* row = part + (int64_t)blockIdx.x * nbins;
  for (int i = threadIdx.x; i < nb * n_catch; i += kBlock) row[i] = series_bins[i];
}

// out[e] = sum over workgroups b of part[b][e], e < nent = nb * n_catch (the
// used front of a row of row_len = kSeriesBatch * n_catch): 16 entries per
// workgroup, each summed by 16 threads over the rows b = r, r + 16, ... in
// order and then pairwise (k_diag_reduce's shape, 16 entries wide so that a
// row is read in 128-byte pieces).
__global__ __launch_bounds__(kBlock) void k_series_reduce(const double* __restrict__ part, int nblocks, int row_len,
                                                          int nent, double* __restrict__ out) {
  __shared__ double red[16][17];
  const int x = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + x;
  double v = 0.0;
  if (e < nent)
    for (int b = r; b < nblocks; b += 16) v += part[(int64_t)b * row_len + e];
  red[r][x] = v;
  __syncthreads();
  for (int s = 8; s > 0; s >>= 1) {
    if (r < s) red[r][x] += red[r + s][x];
    __syncthreads();
  }
  if (r == 0 && e < nent) out[e] = red[0][x];
}
