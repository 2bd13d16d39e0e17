// rtc_mash_merge.h -- Mash's union-truncated pairwise estimator on the device, shared by pair_mash_kernel (rtc_pairs.hip) and
// the --db search (rtc_rep_topk.hip): merge the two ascending lists, stop after `sketch_size` elements of the UNION;
// *common = shared elements among them, *denom = union elements seen (sketch_size unless both lists run out first).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <typename T>
__device__ __forceinline__ void rtc_mash_merge(const T* __restrict__ a, uint32_t na, const T* __restrict__ b, uint32_t nb,
                                               uint32_t sketch_size, uint32_t* common, uint32_t* denom) {
  uint32_t i = 0, j = 0, c = 0, d = 0;
  while (d < sketch_size && i < na && j < nb) {
    const T va = a[i], vb = b[j];
    if (va < vb) i++;
    else if (vb < va) j++;
    else { c++; i++; j++; }
    d++;
  }
  if (d < sketch_size) {  // one list exhausted: the rest of the other one still belongs to the union
    const uint32_t rest = (i < na ? na - i : 0) + (j < nb ? nb - j : 0);
    d += rest < sketch_size - d ? rest : sketch_size - d;
  }
  *common = c;
  *denom = d;
}
