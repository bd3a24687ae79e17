// photon_sort.hpp - what photon_trace.hip and photon_sort.hip share: the sort's scratch (owned by the scene, grown on demand)
// and the two entry points.  ONE definition of the struct for both translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "photon_pool.hpp"

// Scratch of the sort, owned by the caller (the scene) and grown on demand: with it a sort allocates nothing and never
// waits for the host -- photon_trace stays asynchronous on its stream when a lens-major launch has to order a new range.
// Outside the block cache (device_malloc): a regrow hands the old blocks to the runtime, whose free waits for the device.
struct photon_sort_scratch {
    photon::DeviceBuffer<unsigned> box, keys, tmp;      // keys: 2 x idx.n (in, out); tmp: the counts of one radix pass
    photon::DeviceBuffer<int> idx;
};

// perm_out[k] (device, n entries) = index, in the CALLER's source numbering, of the k-th source of
// [first, first + n) in Morton order.  x, y: device pointers to the whole source arrays.  Asynchronous on
// `stream`; allocates only when the scratch has to grow.  Returns 0 or a HIP error code.
int photon_morton_order(const float *d_x, const float *d_y, int first, long long n, int *d_perm_out, hipStream_t stream,
                        photon_sort_scratch *scratch);
