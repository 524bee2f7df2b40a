// nk_fft_g.hip -- the grouped twins of the sandwich's first and final pass (nk_hartley_sandwich_group, include/niftyk.h) and
// their launchers; see nk_fft_batch.h for the block order.  Same phase functions as the single kernels of nk_fft.hip
// (nk_fft3.h, nk_fft2.h), called with the member's fuse record, work array and member-local workgroup index: the same bits.
// A translation unit of its own because every twin is another instantiation of a heavy template.
#include <hip/hip_runtime.h>

#include "nk_fft_batch.h"

// first pass: QUAD workgroups of prologue class 5 (AMP_JVP on octant fields) or 8 (the same with the pending CG direction
// update).  `per` = (na/2 + 1) * (nm/2 + 1) workgroups per member; the surplus of the last group of eight leaves at once.
template <typename T, int H, int PC>
__device__ __forceinline__ void nk_group_contig3(const NkPass3& p, const NkGroupFuse& fa, const NkGroupWork& wa, int count, int64_t per,
                                                 const C2<T>* __restrict__ tw, const C2<T>* __restrict__ twr, unsigned char* smem) {
  int64_t member, local;
  nk_group_decode((int64_t)blockIdx.x, count, member, local);
  if (local >= per) return;
  DeviceExec<T, Contig3Tile<T, H>::SC::E> ex;
  nk_contig3_body<T, H, 4, PC, true>(ex, p, fa.f[member], local, (T*)smem, tw, twr, (C2<T>*)wa.work[member], 0);
}
template <typename T, int H, int PC>
__global__ void __launch_bounds__((Contig3Tile<T, H>::QTHREADS))
    k3_contig_quad_g(NkPass3 p, NkGroupFuse fa, NkGroupWork wa, int count, int64_t per, const C2<T>* __restrict__ tw,
                     const C2<T>* __restrict__ twr) {
  extern __shared__ __align__(16) unsigned char smem[];
  nk_group_contig3<T, H, PC>(p, fa, wa, count, per, tw, twr, smem);
}
// the same under the occupancy cap of its class (k3_contig_quad_w)
template <typename T, int H, int PC, int MAXW>
__global__ void __launch_bounds__((Contig3Tile<T, H>::QTHREADS)) __attribute__((amdgpu_waves_per_eu(1, MAXW)))
    k3_contig_quad_gw(NkPass3 p, NkGroupFuse fa, NkGroupWork wa, int count, int64_t per, const C2<T>* __restrict__ tw,
                      const C2<T>* __restrict__ twr) {
  extern __shared__ __align__(16) unsigned char smem[];
  nk_group_contig3<T, H, PC>(p, fa, wa, count, per, tw, twr, smem);
}
template <typename T, int H, int PC>
static constexpr auto nk_group_quad_kernel() {
  if constexpr (nk_quad_max_waves<T, PC>() < 8)
    return k3_contig_quad_gw<T, H, PC, nk_quad_max_waves<T, PC>()>;
  else
    return k3_contig_quad_g<T, H, PC>;
}

template <typename T, int H, int PC>
int nk_group_launch_contig3(const NkPass3& p3, const NkGroupFuse& fa, const NkGroupWork& wa, int count, const C2<T>* tw, const C2<T>* twr,
                            hipStream_t st) {
  using CT = Contig3Tile<T, H>;
  if constexpr (!CT::QUAD_OK) {
    return nk_set_error(NK_ERR_UNSUPPORTED, "grouped first pass: no QUAD build for this length");
  } else {
    const int64_t per = (int64_t)(p3.g.na / 2 + 1) * (p3.g.nm / 2 + 1);
    const int64_t grid = nk_group_grid(per, count);
    if (p3.nblk > 0 || p3.nlines != (int64_t)p3.g.na * p3.g.nm || grid > 0x7fffffffLL)
      return nk_set_error(NK_ERR_UNSUPPORTED, "grouped first pass: one unstaged grid per member");
    NkPass3 pq = p3;
    pq.blk0 = 0;
    pq.dmh = nk_make_div(p3.g.nm / 2 + 1);
    return nk_launch<nk_group_quad_kernel<T, H, PC>()>("k3_contig_quad_g", dim3((unsigned)grid), dim3(CT::QTHREADS), CT::QLDS_BYTES, st, pq, fa,
                                                       wa, count, per, tw, twr);
  }
}

// final pass: the VJP epilogue on line couples with row-mirror pairing (k2_final<T, NL, true, 2, 1>).  A wavefront's reduction
// slot is local * waves + wave in its MEMBER's slot area -- where the single launch puts it (nk_flush_energy /
// nk_flush_wmax take it from blockIdx.x, which here counts the workgroups of all members): the fixed-order folds see the
// same partials at the same places.
__device__ __forceinline__ void nk_group_flush(const NkFuse& f, double acc, float wmax, int64_t local) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t slot = local * ((blockDim.x + 63) >> 6) + wave;
  if (f.value != nullptr && f.value_slots > 0) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0 && slot < f.value_slots) f.value[slot] = acc;
  }
#ifndef NK_WMAX_OFF
  if (f.w8max != nullptr && f.w8 != nullptr && f.value_slots > 0) {
    for (int off = 32; off > 0; off >>= 1) wmax = nk_wmax_join(wmax, __shfl_down(wmax, off, 64));  // NaN / inf survive
    if (lane == 0 && slot < f.value_slots) f.w8max[slot] = (double)wmax;
  }
#endif
}

template <typename T, int NL>
__global__ void __launch_bounds__((FinalTile<T, NL, 2, 2>::THREADS), (nk_final_waves<T, true, 2, FinalTile<T, NL, 2, 2>::THREADS>()))
    k2_final_g(NkPassF p, NkGroupFuse fa, NkGroupWork wa, int count, int64_t per, const C2<T>* __restrict__ tw, int xmap) {
  extern __shared__ __align__(16) unsigned char smem[];
  int64_t member, local;
  nk_group_decode((int64_t)blockIdx.x, count, member, local);
  if (local >= per) return;
  DeviceExec<T, SchedF<T, NL>::E> ex;
  double acc = 0.0;
  float wmax = 0.0f;
  const int64_t blk = xmap ? nk_xcd_contig(local, per) : local;
  nk_final_body<T, NL, FinalTile<T, NL, 2, 2>::TILE, true, 2, 1>(ex, p, fa.f[member], blk, (T*)smem, tw, (const C2<T>*)wa.work[member], &acc,
                                                                &wmax);
  nk_group_flush(fa.f[member], acc, wmax, local);
}

template <typename T, int NL>
int nk_group_launch_final(NkPassF pf, const NkGroupFuse& fa, const NkGroupWork& wa, int count, const C2<T>* tw, hipStream_t st) {
  using CT = FinalTile<T, NL, 2, 2>;
  static_assert(CT::TILE >= 2, "the couple (b0, M - b0) must live in one workgroup");
  if (pf.a_cnt > 0 || pf.g.batch != 1) return nk_set_error(NK_ERR_UNSUPPORTED, "grouped final pass: one unstaged grid per member");
  pf.tiles_per_a = pf.A > 1 ? (pf.M / 2 + 1 + CT::TILE / 2 - 1) / (CT::TILE / 2) : (pf.M + CT::TILE - 1) / CT::TILE;
  pf.blk0 = 0;
  const int64_t per = (int64_t)(pf.A / 2 + 1) * pf.tiles_per_a;
  const int64_t grid = nk_group_grid(per, count);
  if (grid > 0x7fffffffLL) return nk_set_error(NK_ERR_UNSUPPORTED, "too many lines for one launch");
  // every wavefront owns one slot of its member's energy / |w8| areas: never drop a partial silently
  for (int m = 0; m < count; ++m)
    if (fa.f[m].value_slots > 0 && per * ((CT::THREADS + 63) / 64) > fa.f[m].value_slots)
      return nk_set_error(NK_ERR_RUNTIME, "final pass: more wavefronts than reduction slots (nk_value_slot_count)");
  return nk_launch<k2_final_g<T, NL>>("k2_final_g", dim3((unsigned)grid), dim3(CT::THREADS), CT::LDS_BYTES, st, pf, fa, wa, count, per, tw,
                                      nk_knobs().xmap & 4);
}

#define NK_CASE(NN)                                                                                                                       \
  template int nk_group_launch_contig3<float, NN, 5>(const NkPass3&, const NkGroupFuse&, const NkGroupWork&, int, const C2<float>*,        \
                                                     const C2<float>*, hipStream_t);                                                      \
  template int nk_group_launch_contig3<float, NN, 8>(const NkPass3&, const NkGroupFuse&, const NkGroupWork&, int, const C2<float>*,        \
                                                     const C2<float>*, hipStream_t);                                                      \
  template int nk_group_launch_contig3<double, NN, 5>(const NkPass3&, const NkGroupFuse&, const NkGroupWork&, int, const C2<double>*,      \
                                                      const C2<double>*, hipStream_t);                                                    \
  template int nk_group_launch_contig3<double, NN, 8>(const NkPass3&, const NkGroupFuse&, const NkGroupWork&, int, const C2<double>*,      \
                                                      const C2<double>*, hipStream_t);                                                    \
  template int nk_group_launch_final<float, NN>(NkPassF, const NkGroupFuse&, const NkGroupWork&, int, const C2<float>*, hipStream_t);      \
  template int nk_group_launch_final<double, NN>(NkPassF, const NkGroupFuse&, const NkGroupWork&, int, const C2<double>*, hipStream_t);
NK_FAST_SIZES(NK_CASE)
#undef NK_CASE
