// tfg_aggregate.hpp -- per-cell time aggregates of history planes, device side (gfx950).
//
// Included by tfg_engine.hip after the history layout (kNumHist, H_*), kBlock
// and npmax / npmin (tfg_physics.hpp); the C ABI entry point
// (tfg_cell_aggregate) lives there.
#pragma once

// ---------------------------------------------------------------------------
// Cell aggregates (tfg_cell_aggregate): for one history field, nslots
// consecutive ring slots and every cell i < n, with v_j the cell's value in
// slot j of the call (the engine's element type R), a left fold in slot order:
//   sum   (fp64)   sum  = sum + (double)v_j
//   vmax  (R)      vmax = np.maximum(vmax, v_j)     NaN-propagating (npmax)
//   vmin  (R)      vmin = np.minimum(vmin, v_j)     NaN-propagating (npmin)
//   count (int32)  count += ((double)v_j > threshold)   a NaN is never counted
// starting from +0.0, v_0, v_0 and 0 (init) or from what the buffers hold.
// What a caller of the reference gets from summing or inspecting get_value's
// outputs step by step (examples/run_topoflow_glacier.py:64-115), for every
// cell of a grid and every step still in the history, without a plane leaving
// the device.
//
// There is no partial sum of a batch that is added afterwards, and no
// fast-math flag in the build: the written order is the executed order, so a
// period folded by several calls equals one call over all its slots bit for
// bit, and both equal a numpy loop over the planes in step order.
//
// Shape: a pure stream.  Workgroups own whole, aligned tiles of kBlock * V
// cells (k_forcing_expand's partition); a lane holds V consecutive cells, V =
// 4 (float) or 2 (double), so every history load is 16 bytes per lane and 1 KiB
// per wave instruction.  The slots are taken in batches of kAggBatch, a whole
// batch's loads issued before the first is folded (k_catch_series' eight); the
// slots left over after the full batches go in pieces of 4, 2 and 1, each
// again with all its loads in flight and none issued twice.  An accumulator is
// loaded once, ahead of the first batch, only when the call continues it
// (init == 0), and stored once after the last slot; a statistic whose pointer
// is null is neither loaded nor stored.  Bytes per cell and call:
//   nslots * sizeof(R) + [sum] (8 + 8) + [vmax] 2 sizeof(R) + [vmin] 2 sizeof(R)
//   + [count] (4 + 4),    the read half of each pair absent with init.
//
// Addressing.  History planes are 256-byte aligned and n_pad >= round_up(n, 64)
// cells long, so the 16-byte load of a lane whose first cell is below n is
// aligned and inside its plane even on the ragged last vector; what it reads
// past n is folded and dropped.  Lanes whose first cell is at or past n do
// nothing.  The accumulators are the caller's, exactly n elements each: a
// buffer that is 16-byte aligned (bit in `vec`) is loaded and stored V cells at
// a time on every vector that lies wholly below n, and cell by cell, each cell
// tested against n, on the last ragged vector or when the buffer is not
// aligned.  No element at or past n is touched in either form.  Cell indices
// are 64-bit.  No LDS, no atomics, no cross-lane traffic.
constexpr int kAggBatch = 8;         // history slots in flight per lane
constexpr int kAggMaxBlocks = 2048;  // 8 workgroups per CU

// Bits of k_cell_aggregate's `vec`: the buffer is 16-byte aligned.
enum { kAggVecSum = 1, kAggVecMax = 2, kAggVecMin = 4, kAggVecCount = 8 };

// Workgroups of a k_cell_aggregate launch over n cells, v cells per lane; a
// workgroup takes more than one trip of its tile loop above
// kAggMaxBlocks * kBlock * v cells.
inline int aggregate_blocks(int64_t n, int v) {
  const int64_t tile = (int64_t)kBlock * v;
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + tile - 1) / tile, kAggMaxBlocks));
}

template <int B> struct AggPiece { static constexpr int value = B; };

// plane: the field's plane of history slot 0 (hist + field_index * n_pad);
// slot_stride = kNumHist * n_pad elements.  Slot j of the call is ring slot
// hist0 + j, less hist_depth when that passes the end (0 <= hist0 < hist_depth,
// 1 <= nslots <= hist_depth).  sum, vmax, vmin, cnt: [n] each or null.
template <class R>
__global__ __launch_bounds__(kBlock) void k_cell_aggregate(const R* __restrict__ plane, int64_t slot_stride, int hist_depth,
                                                           int hist0, int nslots, int64_t n, double* __restrict__ sum,
                                                           R* __restrict__ vmax, R* __restrict__ vmin,
                                                           int32_t* __restrict__ cnt, double threshold, int init, int vec) {
  constexpr int V = 16 / (int)sizeof(R);
  constexpr int kTile = kBlock * V;
  typedef R vecR __attribute__((ext_vector_type(V)));
  typedef int32_t vecI __attribute__((ext_vector_type(V)));
  typedef double vecD __attribute__((ext_vector_type(2)));  // 16 bytes: V / 2 of them per lane
  const bool do_sum = sum != nullptr, do_max = vmax != nullptr, do_min = vmin != nullptr, do_cnt = cnt != nullptr;
  const int64_t ntiles = (n + kTile - 1) / kTile;
  const int64_t t0 = (int64_t)blockIdx.x * ntiles / gridDim.x, t1 = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t i0 = t * kTile + (int64_t)threadIdx.x * V;  // the lane's first cell, a multiple of V
    if (i0 >= n) continue;
    const bool full = i0 + V <= n;
    double s[V];
    R mx[V], mn[V];
    int32_t c[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      s[k] = 0.0;
      mx[k] = mn[k] = (R)0;
      c[k] = 0;
    }
    if (!init) {  // continue from the buffers: each read once, ahead of the planes
      if (do_sum) {
        if (full && (vec & kAggVecSum)) {
#pragma unroll
          for (int k = 0; k < V; k += 2) {
            const vecD x = *reinterpret_cast<const vecD*>(sum + i0 + k);
            s[k] = x[0];
            s[k + 1] = x[1];
          }
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (i0 + k < n) s[k] = sum[i0 + k];
        }
      }
      if (do_max) {
        if (full && (vec & kAggVecMax)) {
          const vecR x = *reinterpret_cast<const vecR*>(vmax + i0);
#pragma unroll
          for (int k = 0; k < V; ++k) mx[k] = x[k];
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (i0 + k < n) mx[k] = vmax[i0 + k];
        }
      }
      if (do_min) {
        if (full && (vec & kAggVecMin)) {
          const vecR x = *reinterpret_cast<const vecR*>(vmin + i0);
#pragma unroll
          for (int k = 0; k < V; ++k) mn[k] = x[k];
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (i0 + k < n) mn[k] = vmin[i0 + k];
        }
      }
      if (do_cnt) {
        if (full && (vec & kAggVecCount)) {
          const vecI x = *reinterpret_cast<const vecI*>(cnt + i0);
#pragma unroll
          for (int k = 0; k < V; ++k) c[k] = x[k];
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (i0 + k < n) c[k] = cnt[i0 + k];
        }
      }
    }
    const R* const cell = plane + i0;
    // B slots from slot j0 of the call: every load issued, then folded in slot order
    auto piece = [&](auto tag, int j0) {
      constexpr int B = decltype(tag)::value;
      vecR x[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        int slot = hist0 + j0 + b;
        slot -= slot >= hist_depth ? hist_depth : 0;
        x[b] = *reinterpret_cast<const vecR*>(cell + (int64_t)slot * slot_stride);
      }
      if (init && j0 == 0) {  // vmax and vmin start from v_0
#pragma unroll
        for (int k = 0; k < V; ++k) mx[k] = mn[k] = x[0][k];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const R v = x[b][k];
          if (do_sum) s[k] += (double)v;
          if (do_max) mx[k] = tfg::npmax(mx[k], v);
          if (do_min) mn[k] = tfg::npmin(mn[k], v);
          if (do_cnt) c[k] += (double)v > threshold ? 1 : 0;
        }
      }
    };
    int j0 = 0;
    for (; j0 + kAggBatch <= nslots; j0 += kAggBatch) piece(AggPiece<kAggBatch>{}, j0);
    if (nslots - j0 >= 4) { piece(AggPiece<4>{}, j0); j0 += 4; }
    if (nslots - j0 >= 2) { piece(AggPiece<2>{}, j0); j0 += 2; }
    if (nslots - j0 >= 1) piece(AggPiece<1>{}, j0);

    if (do_sum) {
      if (full && (vec & kAggVecSum)) {
#pragma unroll
        for (int k = 0; k < V; k += 2) {
          vecD x;
          x[0] = s[k];
          x[1] = s[k + 1];
          *reinterpret_cast<vecD*>(sum + i0 + k) = x;
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (i0 + k < n) sum[i0 + k] = s[k];
      }
    }
    if (do_max) {
      if (full && (vec & kAggVecMax)) {
        vecR x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = mx[k];
        *reinterpret_cast<vecR*>(vmax + i0) = x;
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (i0 + k < n) vmax[i0 + k] = mx[k];
      }
    }
    if (do_min) {
      if (full && (vec & kAggVecMin)) {
        vecR x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = mn[k];
        *reinterpret_cast<vecR*>(vmin + i0) = x;
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (i0 + k < n) vmin[i0 + k] = mn[k];
      }
    }
    if (do_cnt) {
      if (full && (vec & kAggVecCount)) {
        vecI x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = c[k];
        *reinterpret_cast<vecI*>(cnt + i0) = x;
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (i0 + k < n) cnt[i0 + k] = c[k];
      }
    }
  }
}
