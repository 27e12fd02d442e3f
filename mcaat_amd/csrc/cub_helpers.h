// cub_helpers.h — the hipcub calls several files make, on with_cub_temp. Included after
// <hipcub/hipcub.hpp> by the files that use hipcub (internal.h also serves files that must not pull
// hipcub in). Header templates: every file instantiates its own hipcub kernels.
#pragma once
#include "internal.h"

namespace mcaat {

// out[i] = in[0] + ... + in[i - 1]. The pointers go to hipcub as the caller types them (a pointer
// to const and one to non-const name different hipcub kernels with the same code)
template <class In, class Out>
void excl_scan(hipStream_t st, In *in, Out *out, uint64_t n) {
    with_cub_temp([&](void *t, size_t &tmp) {
        return hipcub::DeviceScan::ExclusiveSum(t, tmp, in, out, (size_t)n, st);
    });
}

// (key, value) pairs ascending by the low `bits` bits of the key
template <class K, class V>
void sort_pairs(hipStream_t st, const K *keys_in, K *keys_out, const V *vals_in, V *vals_out, uint64_t n, int bits) {
    with_cub_temp([&](void *t, size_t &tmp) {
        return hipcub::DeviceRadixSort::SortPairs(t, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, bits, st);
    });
}

}  // namespace mcaat
