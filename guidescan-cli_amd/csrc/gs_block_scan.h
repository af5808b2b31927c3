/* gs_block_scan.h -- the scan across the lanes of one workgroup that the tile kernels of the device readers share
 * (gs_fasta.hip, gs_kmersfile.hip) */
#ifndef GS_BLOCK_SCAN_H
#define GS_BLOCK_SCAN_H

/* Scan of one value per lane in LDS, the lane's value standing at index `at` (a permutation of 0 .. THREADS-1): -> the
 * combination of the values at the indices below `at` (`none` at index 0); *total: of all of them.  lds holds THREADS
 * values and is free again on return. */
template <uint32_t THREADS, class T, class Op>
__device__ __forceinline__ T gs_block_scan(T *lds, const T &v, uint32_t at, Op op, const T &none, T *total) {
  lds[at] = v;
  __syncthreads();
  for (uint32_t d = 1; d < THREADS; d <<= 1) {
    T x = lds[at];
    if (at >= d) x = op(lds[at - d], x);
    __syncthreads();
    lds[at] = x;
    __syncthreads();
  }
  const T r = at ? lds[at - 1] : none;
  if (total) *total = lds[THREADS - 1];
  __syncthreads();
  return r;
}

#endif
