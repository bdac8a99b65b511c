// Validated adaptation on the device: the per-step decisions of adapt.py:366-396 (OOD gate, reservoir offer of
// utils/stereo_reservoir.py, update or not) and the copy of a stored pair into its reservoir slot.  With these two and the gated
// clip + Adam of optim.hip an IN_PROGRESS step of the VS / ER modes needs no host read-back and replays as one hipGraph
// (adaptive_stereo/control.py).  Every entry point only enqueues; gating is an early return.
#include "as_common.h"

// One wave.  Every lane reads the same scalars and takes the same branches; the duplicate search is lane-strided; lane 0 writes.
// state = [size, offers, adds, updates] (int64), out3 = [novel, slot, update] (int32).
__global__ __launch_bounds__(64) void adapt_gate_kernel(const float* __restrict__ fcs_smoothed, const float* __restrict__ loss,
                                                         const int32_t* __restrict__ batch_idx, const double* __restrict__ u,
                                                         double threshold, int capacity, int gate_enabled, int adapting,
                                                         int64_t* __restrict__ state, int32_t* __restrict__ indices,
                                                         float* __restrict__ values, int32_t* __restrict__ out3) {
  const int lane = threadIdx.x;
  int64_t size = state[0], offers = state[1], adds = state[2], updates = state[3];
  // strict < in double, as float(tensor) < threshold on the host: a NaN is never novel
  const int novel = (gate_enabled != 0) && ((double)fcs_smoothed[0] < threshold);
  int slot = -1;
  if (novel) {                                     // wave-uniform
    offers += 1;
    const int32_t idx = batch_idx[0];
    int dup = 0;
    for (int64_t i = lane; i < size; i += 64) dup |= (indices[i] == idx);
    dup = __any(dup);
    if (!dup) {
      if (size < capacity) {
        slot = (int)size;
        if (lane == 0) indices[size] = idx;
        size += 1;
      } else {
        // random.randint(1, offers) from one uniform double: 1 + min(int(u * offers), offers - 1); a replacement changes
        // neither `indices` nor `size` (the reference's reservoir keeps the replaced pair's index in its set)
        int64_t k = (int64_t)(u[0] * (double)offers);
        if (k > offers - 1) k = offers - 1;
        const int64_t r = 1 + k;
        if (r <= capacity) slot = (int)(r - 1);
      }
    }
    if (slot >= 0) adds += 1;
  }
  const int update = (adapting != 0) && slot < 0;
  updates += update;
  if (lane == 0) {
    if (slot >= 0) values[slot] = loss[0];
    state[0] = size; state[1] = offers; state[2] = adds; state[3] = updates;
    out3[0] = novel; out3[1] = slot; out3[2] = update;
  }
}

extern "C" int as_adapt_gate(const float* fcs_smoothed, const float* loss, const int32_t* batch_idx, const double* u,
                             double threshold, int capacity, int gate_enabled, int adapting, int64_t* state,
                             int32_t* indices, float* values, int32_t* out3, void* stream) {
  AS_CHECK_ARG(fcs_smoothed && loss && batch_idx && u && state && indices && values && out3 && capacity >= 1,
               "as_adapt_gate: bad argument");
  AS_CHECK_ARG((((uintptr_t)u | (uintptr_t)state) & 7) == 0, "as_adapt_gate: u and state must be 8-byte aligned");
  hipLaunchKernelGGL(adapt_gate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, fcs_smoothed, loss, batch_idx, u, threshold,
                     capacity, gate_enabled, adapting, state, indices, values, out3);
  AS_CHECK_LAUNCH("as_adapt_gate");
  return AS_OK;
}

// blockIdx.y = 0: left, 1: right.  A refused slot returns from every workgroup before the first write.  16-byte loads and
// stores when source and destination row are both 16-byte aligned (the row's alignment depends on slot * n), else floats.
#define RS_MAX_BLOCKS 1024
__global__ __launch_bounds__(256) void reservoir_store_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                               long n, const int32_t* __restrict__ slot_dev, int capacity,
                                                               float* __restrict__ buf_left, float* __restrict__ buf_right) {
  const int slot = slot_dev[0];
  if (slot < 0 || slot >= capacity) return;
  const float* __restrict__ src = blockIdx.y ? right : left;
  float* __restrict__ dst = (blockIdx.y ? buf_right : buf_left) + (long)slot * n;
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const long n4 = n >> 2;
    const f32x4* __restrict__ s4 = reinterpret_cast<const f32x4*>(src);
    f32x4* __restrict__ d4 = reinterpret_cast<f32x4*>(dst);
    for (long i = tid; i < n4; i += stride) d4[i] = s4[i];
    for (long i = (n4 << 2) + tid; i < n; i += stride) dst[i] = src[i];       // tail: at most 3 floats
  } else {
    for (long i = tid; i < n; i += stride) dst[i] = src[i];
  }
}

extern "C" int as_reservoir_store(const float* left, const float* right, int64_t n, const int32_t* slot_dev, int capacity,
                                  float* buf_left, float* buf_right, void* stream) {
  AS_CHECK_ARG(left && right && slot_dev && buf_left && buf_right && n > 0 && capacity >= 1, "as_reservoir_store: bad argument");
  AS_CHECK_ARG((((uintptr_t)left | (uintptr_t)right | (uintptr_t)buf_left | (uintptr_t)buf_right) & 3) == 0,
               "as_reservoir_store: 4-byte aligned tensors");
  long nb = (n + 1023) / 1024;                      // one 16-byte access per thread and trip
  if (nb > RS_MAX_BLOCKS) nb = RS_MAX_BLOCKS;
  hipLaunchKernelGGL(reservoir_store_kernel, dim3((int)nb, 2), dim3(256), 0, (hipStream_t)stream, left, right, (long)n, slot_dev,
                     capacity, buf_left, buf_right);
  AS_CHECK_LAUNCH("as_reservoir_store");
  return AS_OK;
}

// The reference's utils/stereo_priority_queue.py as one wave: keeps the `capacity` smallest keys (key = value for a min heap,
// -value for a max heap).  Every lane reads the same scalars and takes the same branches; the duplicate search and the search for
// the worst member are lane-strided; lane 0 writes.  state = [size, offers, adds] (int64).
__global__ __launch_bounds__(64) void pq_offer_kernel(const float* __restrict__ value, const int32_t* __restrict__ index,
                                                       int capacity, int min_heap, int64_t* __restrict__ state,
                                                       int32_t* __restrict__ indices, float* __restrict__ keys,
                                                       int32_t* __restrict__ out_slot) {
  const int lane = threadIdx.x;
  int64_t size = state[0];
  const float v = value[0];
  const float key = min_heap ? v : -v;
  const int32_t idx = index[0];
  int slot = -1;
  if (key == key) {                                // a NaN is refused: it has no place in the order (wave-uniform)
    int dup = 0;
    for (int64_t i = lane; i < size; i += 64) dup |= (indices[i] == idx);
    if (!__any(dup)) {
      if (size < capacity) {
        slot = (int)size;
        size += 1;
      } else {
        // the worst member: the maximum by (key, index)
        float wk = 0.f;
        int32_t wi = 0;
        int ws = -1;
        for (int64_t i = lane; i < size; i += 64) {
          const float k = keys[i];
          const int32_t j = indices[i];
          if (ws < 0 || k > wk || (k == wk && j > wi)) { wk = k; wi = j; ws = (int)i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float k = __shfl_xor(wk, o, 64);
          const int32_t j = __shfl_xor(wi, o, 64);
          const int s = __shfl_xor(ws, o, 64);
          if (s >= 0 && (ws < 0 || k > wk || (k == wk && j > wi))) { wk = k; wi = j; ws = s; }
        }
        if (key < wk) slot = ws;                   // strictly better only: an offer equal to the worst key is refused
      }
    }
  }
  if (lane == 0) {
    if (slot >= 0) { indices[slot] = idx; keys[slot] = key; }
    state[0] = size; state[1] += 1; state[2] += (slot >= 0);
    out_slot[0] = slot;
  }
}

extern "C" int as_pq_offer(const float* value, const int32_t* index, int capacity, int min_heap, int64_t* state,
                           int32_t* indices, float* keys, int32_t* out_slot, void* stream) {
  AS_CHECK_ARG(value && index && state && indices && keys && out_slot && capacity >= 1, "as_pq_offer: bad argument");
  AS_CHECK_ARG(((uintptr_t)state & 7) == 0, "as_pq_offer: state must be 8-byte aligned");
  hipLaunchKernelGGL(pq_offer_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, value, index, capacity, min_heap, state, indices,
                     keys, out_slot);
  AS_CHECK_LAUNCH("as_pq_offer");
  return AS_OK;
}
