// tfg_bands.hpp -- per-catchment, per-elevation-band sums and counts of history
// planes, device side (gfx950).
//
// Included by tfg_engine.hip after tfg_series.hpp (series_wave_sums,
// k_series_reduce, kSeriesMaxBlocks, kSeriesScratchMax); the C ABI entry point
// (tfg_band_series) lives in tfg_engine.hip.
#pragma once

// ---------------------------------------------------------------------------
// Band series (tfg_band_series): for one history field, a batch of NB history
// slots and the keys (c, k) = (catchment of the cell, elevation band of the
// cell), K = n_catch * n_bands of them,
//   sum  [slot][c][k] = sum over the cells i < n of (c, k) of hist[slot][field][i]   fp64
//   count[slot][c][k] = number of those cells with (double)value > threshold
//   cells      [c][k] = number of cells of (c, k)                   (the hypsometry)
// What a caller of the reference that bins its outputs by elevation gets from
// a get_value loop over every step, without the planes leaving the device.
//
// Key.  The band is a second key next to the catchment id, computed in the
// kernel from the two rasters the handle holds: a lane loads catch_id[i] and
// elev[i] once per cell and batch (8 B per cell with the fp32 engine's
// elevation, 12 B with the fp64 engine's), widens the elevation to fp64
// (exact) and finds k with edges[k] <= z < edges[k+1] by a branch-free binary
// search, seven LDS reads over the edges padded to 127 entries with NaN: pos
// counts the edges <= z (numpy's searchsorted(edges, z, side="right")), a NaN
// pad or a NaN z compares false, and the cell is in band pos - 1 when that is
// in 0 .. n_bands-1.  There is no per-cell key plane (268 MB at 8192^2, stale
// whenever a raster is set).  A cell in no band, and a cell at or past n
// (which loads cell n-1: an in-bounds address, no branch around a load), is
// inactive: it contributes a selected 0 to sums and a false to ballots.
//
// Shape: k_catch_series's.  Workgroups own whole, aligned chunks of kBlock
// cells; per chunk a lane issues all its loads (id, elevation, the value in
// every position of the batch) before the first is used, and the next chunk's
// before the current chunk is reduced.  Per wave, before its turn at the bins:
//   one key in the wave (most waves of a smooth raster): as the series
//           kernel's one id -- the values, 0 in an inactive lane, through the
//           fixed butterfly band_wave_sums (pairs xor 32, 16, 8, 4, 2, 1 in
//           that order for every NB), one lane per position holding the sum;
//           count = __popcll(__ballot(active && value > threshold)) per
//           position, no butterfly; cells = __popcll(active).
//   many keys (the normal case here, unlike the series kernel's: a wave of 64
//           cells of uniform-random elevations over 64 bands holds 31 to 43
//           keys, and on smooth terrain a wave often straddles a band edge):
//           the ballot / leader loop makes a trip per distinct key, but a
//           cheap one -- a lane learns its rank among the lanes of its key and
//           the number of lanes of smaller keys, no value moves.  Then every
//           lane sends its cell to its place in key order (ds_permute: the
//           inactive lanes behind the active ones, under key -1 with zeros),
//           and a segmented inclusive scan over the sorted lanes (steps 1, 2,
//           4, 8, 16, 32; a lane adds the value d lanes down when that lane's
//           key is its own, which between sorted lanes means the same
//           segment) leaves each key's sum in the key's last lane: six levels
//           whatever the number of keys, where a butterfly pass per key
//           (the series kernel's loop) takes six per key.  Counts: the
//           above-threshold bits travel with the cell, and the key's last
//           lane counts the ballot over its segment's lanes; cells = its
//           rank + 1.  The order of the additions is a function of the keys
//           in the wave alone.
// In its turn (wave order: the four waves share the bins) a wave adds to the
// LDS bins: one lane per position, or with many keys each key's last lane (no
// two lanes add to one bin).  cells is accumulated in a call's first batch only.
//
// Bins and batch.  A workgroup's LDS holds, per position and key, an fp64 sum
// and an int32 count (12 B), plus an int32 cell count per key and the 1 KiB
// of edges.  The positions per launch follow from K alone (band_batch), so
// that sums and counts stay at or under 48 KiB and two to three workgroups
// fit a CU's 160 KiB:
//   K <=  512: 8 slots per launch   (<= 48 KiB + 2 KiB + 1 KiB)
//   K <= 1024: 4                    (<= 48 KiB + 4 KiB + 1 KiB)
//   K <= 2048: 2                    (<= 48 KiB + 8 KiB + 1 KiB)
// NB = 0 is the cells-only launch (sum == count == NULL): no plane is read.
//
// Bytes (algorithmic, fp32 engine): per cell 8 B of id and elevation per
// batch plus 4 B per slot, i.e. per cell and slot 4 + 8 / NB: 5, 6 and 8 B in
// the three classes (k_catch_series: 4.5 B).
//
// No floating-point atomics, no dependence on dispatch order: a call's result
// is bit-reproducible.  Every position goes through the same operations on its
// own values alone -- the positions of a batch share only the keys and the
// control flow -- and the batch size and the workgroup count depend on n and K
// only, so a (slot, catchment, band) entry does not depend on which other
// slots share the call or where in a batch it sits.  A short last batch loads
// its last slot again in the unused positions and stores no row for them.  A
// NaN value reaches exactly the sum of its own (slot, catchment, band): a
// value is added only within its key's segment (a select, never a product),
// other positions never see it, and NaN > threshold is false.
//
// Partials and fold.  A workgroup ends by storing its bins as one row of
// partials: fp64 sums [NB][K] in one buffer, int32 counts [NB][K] and cells [K]
// in another (a workgroup sees fewer than 2^31 cells).  k_series_reduce folds
// the sums over the workgroups in its fixed order; k_band_reduce_int folds the
// integers into int64 likewise.  Both buffers are the history readers' shared
// scratch, reserved by each call for its own K; band_blocks() caps the
// workgroups at kSeriesMaxBlocks and so that both together stay at or under
// kSeriesScratchMax (64 MiB): a row is K * (12 * NB + 4) bytes.
//
// Longest chain of dependent fp64 additions of one sum: 6 (butterfly or scan) +
// 4 * chunks per workgroup (the bins) + workgroups / 16 + 4 (the fold).  At
// 8192^2 cells (262144 chunks), at the largest K of each class:
//   K =  512 (NB 8): 1310 workgroups, 201 chunks: 6 + 804 + 82 + 4 = 896
//   K = 1024 (NB 4): 1260 workgroups, 209 chunks: 6 + 836 + 79 + 4 = 925
//   K = 2048 (NB 2): 1170 workgroups, 225 chunks: 6 + 900 + 74 + 4 = 984
// and, e.g., K = 352 (44 catchments x 8 bands): 1906 workgroups, 138 chunks:
// 6 + 552 + 120 + 4 = 682.  The 900 terms that the 1e-13 bound of the tests
// stands on are exceeded at 8192^2 in the upper part of the second class
// (K >= 989) and of the third (K >= 1837), by under 10 %: there the bound is
// 984 * 2^-53 = 1.1e-13.  (The scratch cap sets the workgroups, and the bins
// term is inversely proportional to them.)
constexpr int kBandMaxBands = 64;
constexpr int kBandMaxKeys = 2048;    // n_catch * n_bands of one call
constexpr int kBandEdgePad = 128;     // LDS entries of the edges: 127 searched, NaN past n_bands

struct BandEdges { double e[kBandMaxBands + 1]; };  // passed by value: consumed at the launch

// Slots per launch for K keys.
inline int band_batch(int K) { return K <= 512 ? 8 : K <= 1024 ? 4 : 2; }

// Bytes of a workgroup's row of partials (fp64 sums, int32 counts and cells).
inline int64_t band_row_bytes(int K) { return (int64_t)K * (12 * band_batch(K) + 4); }

// Workgroups of a k_band_series launch over n cells (= rows of partials).
inline int band_blocks(int64_t n, int K) {
  const int64_t chunks = (n + kBlock - 1) / kBlock;
  const int64_t by_scratch = kSeriesScratchMax / band_row_bytes(K);
  return (int)std::max<int64_t>(1, std::min<int64_t>({chunks, (int64_t)kSeriesMaxBlocks, by_scratch}));
}

// Dynamic LDS of a launch with NB positions.
inline size_t band_lds_bytes(int NB, int K) { return (size_t)NB * K * 12 + kBandEdgePad * 8 + (size_t)K * 4; }

// The sums of a wave's NB values per lane, by series_wave_sums's butterfly cut
// to NB positions: the lane bits 5.. select the position a lane keeps while
// positions remain, and the rest of xor 32, 16, 8, 4, 2, 1 sums that one.  For
// every NB and position the same pairs in the same order.  Returns, in every
// lane, the wave's sum of position lane / (64 / NB).
template <int NB>
__device__ __forceinline__ double band_wave_sums(const double (&v)[NB], int lane) {
  static_assert(NB == 8 || NB == 4 || NB == 2, "positions fold over the lane bits 5, 4, 3");
  if constexpr (NB == 8) {
    return series_wave_sums(v, lane);
  } else if constexpr (NB == 4) {
    const bool h5 = lane & 32, h4 = lane & 16;
    double a[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) a[j] = (h5 ? v[2 + j] : v[j]) + __shfl_xor(h5 ? v[j] : v[2 + j], 32);
    double t = (h4 ? a[1] : a[0]) + __shfl_xor(h4 ? a[0] : a[1], 16);
    t += __shfl_xor(t, 8);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 1);
    return t;
  } else {
    const bool h5 = lane & 32;
    double t = (h5 ? v[1] : v[0]) + __shfl_xor(h5 ? v[0] : v[1], 32);
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 8);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 1);
    return t;
  }
}

constexpr int kBandSum = 1, kBandCount = 2, kBandCells = 4;  // what a launch accumulates and stores

// plane, slot_stride, hist_depth, slot0, nb: as k_catch_series (position s
// reads slot (slot0 + min(s, nb - 1)) % hist_depth).  elev: the handle's
// elevation plane [n_pad], engine type.  K = n_catch * n_bands.
// part_sum: [gridDim.x][NB][K] fp64; part_int: [gridDim.x][NB * K + K] int32
// (counts, then cells).  CATCH: an id raster is set; without one every cell is
// in catchment 0.  NB = 0: cells only.
template <class R, bool CATCH, int NB>
__global__ __launch_bounds__(kBlock) void k_band_series(const R* __restrict__ plane, int64_t slot_stride, int hist_depth,
                                                        int slot0, int nb, const int32_t* __restrict__ catch_id,
                                                        const R* __restrict__ elev, const BandEdges edges, int n_bands,
                                                        double thr, int what, int64_t n, int K,
                                                        double* __restrict__ part_sum, int32_t* __restrict__ part_int) {
  constexpr int NV = NB ? NB : 1;
  extern __shared__ __attribute__((aligned(16))) double band_lds[];
  double* const sums = band_lds;                                        // [NB][K]
  double* const edge = band_lds + NB * K;                               // [kBandEdgePad]
  int32_t* const counts = reinterpret_cast<int32_t*>(edge + kBandEdgePad);  // [NB][K]
  int32_t* const cellb = counts + NB * K;                               // [K]
  const int nbins = NB * K;
  for (int i = threadIdx.x; i < nbins; i += kBlock) {
    sums[i] = 0.0;
    counts[i] = 0;
  }
  for (int i = threadIdx.x; i < K; i += kBlock) cellb[i] = 0;
  if (threadIdx.x < kBandEdgePad) {
    const int j = threadIdx.x <= (unsigned)n_bands ? threadIdx.x : n_bands;
    const double ev = edges.e[j];
    edge[threadIdx.x] = threadIdx.x <= (unsigned)n_bands ? ev : __builtin_nan("");
  }
  __syncthreads();

  const bool want_sum = NB && (what & kBandSum), want_count = NB && (what & kBandCount), want_cells = what & kBandCells;
  const R* sp[NV];
#pragma unroll
  for (int s = 0; s < NV; ++s)
    sp[s] = NB ? plane + (int64_t)((slot0 + (s < nb ? s : nb - 1)) % hist_depth) * slot_stride : nullptr;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nchunks = (n + kBlock - 1) / kBlock;
  const int64_t wg = blockIdx.x;
  const int64_t c0 = wg * nchunks / gridDim.x, c1 = (wg + 1) * nchunks / gridDim.x;
  constexpr int kPer = 64 / NV;                        // lanes per position after band_wave_sums
  double* const mybin = sums + (lane / kPer) * K;     // the position this lane holds after band_wave_sums
  const bool writer = (lane % kPer) == 0;
  int32_t* const mycount = counts + (lane < NV ? lane : 0) * K;  // lane s < NB adds position s's count

  // a chunk's loads: the id and the elevation once per cell, then the cell in every position
  auto load = [&](int64_t ch, int& cid, R& z, R (&x)[NV]) {
    const int64_t i = ch * kBlock + threadIdx.x;
    const int64_t il = i < n ? i : n - 1;
    if constexpr (CATCH) cid = catch_id[il]; else cid = 0;
    z = elev[il];
    if constexpr (NB > 0) {
#pragma unroll
      for (int s = 0; s < NV; ++s) x[s] = sp[s][il];
    }
  };
  // the key of a cell, -1 when it is in no band: pos = the edges <= z
  auto key_of = [&](int cid, R z) {
    const double zd = (double)z;
    int pos = 0;
#pragma unroll
    for (int s = 64; s > 0; s >>= 1) pos += (edge[pos + s - 1] <= zd) ? s : 0;
    const int band = pos - 1;
    return (unsigned)band < (unsigned)n_bands ? cid * n_bands + band : -1;
  };
  // the counts of the lanes `mine` above the threshold, position s in lane s
  auto counts_of = [&](bool mine, const R (&x)[NV]) {
    int myc = 0;
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int c = __popcll(__ballot(mine && (double)x[s] > thr));
      myc = lane == s ? c : myc;
    }
    return myc;
  };

  int cid = 0;
  R z = (R)0;
  R x[NV] = {};
  if (c0 < c1) load(c0, cid, z, x);
  for (int64_t ch = c0; ch < c1; ++ch) {
    // the next chunk's loads are in flight while this one is reduced (the last
    // trip loads its own chunk again: no branch around the loads)
    int cid_n;
    R z_n;
    R x_n[NV];
    load(ch + 1 < c1 ? ch + 1 : ch, cid_n, z_n, x_n);
    const int key = key_of(cid, z);
    const bool has = ch * kBlock + threadIdx.x < n && key >= 0;
    const uint64_t active = __ballot(has);
    const int k_first = __shfl(key, active ? __builtin_ctzll(active) : 0);
    // one key in the wave: its sums and counts are formed before the wave's turn
    const bool one_key = __ballot(has && key == k_first) == active;
    double t = 0.0;
    int myc = 0;
    // many keys: the sorted lanes' key, the lanes of that key before this one, and,
    // in the last lane of a key (tail), the key's sums and counts per position
    int skey = -1, srank = 0;
    bool tail = false;
    double ts[NV] = {};
    int tcnt[NV] = {};
    if (one_key && active) {
      if (want_sum) {
        double v[NV];
#pragma unroll
        for (int s = 0; s < NV; ++s) v[s] = has ? (double)x[s] : 0.0;
        if constexpr (NB > 0) t = band_wave_sums<NB>(v, lane);
      }
      if (want_count) myc = counts_of(has, x);
    } else if (active) {
      // the ballot / leader loop, a trip per distinct key: a lane's rank among
      // the lanes of its key, and the lanes of smaller keys
      int rank = 0, below = 0;
      const uint64_t lanes_lt = (1ull << lane) - 1;
      for (uint64_t pending = active; pending;) {
        const int k = __shfl(key, __builtin_ctzll(pending));
        const bool mine = has && (key == k);
        const uint64_t m = __ballot(mine);
        rank = mine ? __popcll(m & lanes_lt) : rank;
        below += (has && k < key) ? __popcll(m) : 0;
        pending &= ~m;
      }
      // every lane sends its cell to its place in key order (a bijection:
      // the inactive lanes go behind the active ones, with key -1 and zeros)
      const int dst = 4 * (has ? below + rank : __popcll(active) + __popcll(~active & lanes_lt));
      skey = __builtin_amdgcn_ds_permute(dst, has ? key : -1);
      srank = __builtin_amdgcn_ds_permute(dst, rank);
      const int k_up = __shfl_down(skey, 1);
      tail = skey >= 0 && (lane == 63 || k_up != skey);
      if (want_sum) {
#pragma unroll
        for (int s = 0; s < NV; ++s) {
          const double v = has ? (double)x[s] : 0.0;
          ts[s] = __hiloint2double(__builtin_amdgcn_ds_permute(dst, __double2hiint(v)),
                                   __builtin_amdgcn_ds_permute(dst, __double2loint(v)));
        }
        // segmented inclusive scan: equal keys are adjacent, so the key d lanes
        // down being this lane's means that all between are
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int k_down = __shfl_up(skey, d);  // every lane takes part: not under the && below
          const bool same = lane >= d && k_down == skey;
#pragma unroll
          for (int s = 0; s < NV; ++s) {
            const double u = __shfl_up(ts[s], d);
            ts[s] = same ? ts[s] + u : ts[s];
          }
        }
      }
      if (want_count) {
        int above = 0;
#pragma unroll
        for (int s = 0; s < NV; ++s) above |= (has && (double)x[s] > thr) ? 1 << s : 0;
        above = __builtin_amdgcn_ds_permute(dst, above);
        const uint64_t seg = ((2ull << lane) - 1) & ~((1ull << (lane - srank)) - 1);  // the key's lanes up to this one
#pragma unroll
        for (int s = 0; s < NV; ++s) tcnt[s] = __popcll(__ballot((above >> s) & 1) & seg);
      }
    }
    for (int turn = 0; turn < kWaves; ++turn) {
      if (wave == turn && active) {
        if (one_key) {
          if (want_sum && writer) mybin[k_first] += t;
          if (want_count && lane < NV) mycount[k_first] += myc;
          if (want_cells && lane == 0) cellb[k_first] += __popcll(active);
        } else if (tail) {  // one lane per key: no two add to the same bin
          if (want_sum) {
#pragma unroll
            for (int s = 0; s < NV; ++s) sums[s * K + skey] += ts[s];
          }
          if (want_count) {
#pragma unroll
            for (int s = 0; s < NV; ++s) counts[s * K + skey] += tcnt[s];
          }
          if (want_cells) cellb[skey] += srank + 1;
        }
      }
      __syncthreads();
    }
    cid = cid_n;
    z = z_n;
#pragma unroll
    for (int s = 0; s < NV; ++s) x[s] = x_n[s];
  }
  // the last turn's barrier (or the one after the zeroing) made the bins visible
  if (want_sum) {
    double* row = part_sum + (int64_t)blockIdx.x * nbins;
    for (int i = threadIdx.x; i < nb * K; i += kBlock) row[i] = sums[i];
  }
  int32_t* irow = part_int + (int64_t)blockIdx.x * (nbins + K);
  if (want_count)
    for (int i = threadIdx.x; i < nb * K; i += kBlock) irow[i] = counts[i];
  if (want_cells)
    for (int i = threadIdx.x; i < K; i += kBlock) irow[nbins + i] = cellb[i];
}

// out[e] = sum over workgroups b of part[b][e], e < nent, int32 partials into
// int64: k_series_reduce's shape and order (integers: any order gives the
// same sum; the shape keeps a row's reads in 64-byte pieces).
__global__ __launch_bounds__(kBlock) void k_band_reduce_int(const int32_t* __restrict__ part, int nblocks, int row_len,
                                                            int nent, int64_t* __restrict__ out) {
  __shared__ int64_t red[16][17];
  const int x = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + x;
  int64_t v = 0;
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
