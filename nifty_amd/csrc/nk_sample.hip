// nk_sample.hip -- LinearInterpolator and RegriddingOperator on device fields (nifty_amd/sampling_operators.py;
// include/niftyk.h "sampling"; docs/SAMPLING.md).  Matrix-free: the per-element bodies of nk_sample.h form the weights in
// registers.  No float atomics: every output is summed by one thread, or by one workgroup with a fixed tree, in an order
// that is a function of the plan only, so results are bit-reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nk_sample.h"
#include "nk_util.h"

namespace {

struct SampleGrid {
  int64_t n[3];
};

// TIMES: one thread per point in SORTED order (neighbouring threads read neighbouring cells); the result goes to the
// point's original index, a streamed store that is not read again here.
template <typename T, int ND>
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_sample_times(SampleGrid g, int64_t npoints, const int64_t* __restrict__ cell,
                                                                  const double* __restrict__ frac, const int64_t* __restrict__ perm,
                                                                  const T* __restrict__ x, T* __restrict__ y) {
  const int64_t k = (int64_t)blockIdx.x * NK_SAMPLE_BLOCK + threadIdx.x;
  if (k >= npoints) return;
  double e[ND];
  for (int a = 0; a < ND; ++a) e[a] = frac[k * ND + a];
  const double acc = nk_sample_gather<T, ND>(g.n, cell[k], e, x);
  const int64_t o = perm[k];
  if ((uint64_t)o < (uint64_t)npoints) __builtin_nontemporal_store((T)acc, y + o);
}

// ADJOINT_TIMES, pass of corner m over the SHORT occupied cells: one thread per occupied cell sums the cell's points in
// list order and adds the sum into acc[cell + m] with a plain read-modify-write.  Within one pass distinct cells write
// distinct outputs (cell -> cell + m mod n is one-to-one); the passes are stream-ordered.
template <typename T, int ND>
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_sample_adjoint_short(SampleGrid g, int64_t npoints, int64_t ncells, int m,
                                                                          const int64_t* __restrict__ cell,
                                                                          const double* __restrict__ frac,
                                                                          const int64_t* __restrict__ perm,
                                                                          const int64_t* __restrict__ cell_start,
                                                                          const T* __restrict__ y, double* __restrict__ acc) {
  const int64_t c = (int64_t)blockIdx.x * NK_SAMPLE_BLOCK + threadIdx.x;
  if (c >= ncells) return;
  int64_t lo = cell_start[c], hi = cell_start[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > npoints ? npoints : hi;
  if (hi <= lo || hi - lo > NK_SAMPLE_LONG) return;
  const double s = nk_sample_cell_sum<T, ND>(frac, perm, y, npoints, m, lo, hi, 1);
  int64_t idx[ND];
  nk_sample_decode<ND>(cell[lo], g.n, idx);
  acc[nk_sample_corner<ND>(idx, g.n, m)] += s;
}

// ... and over the LONG cells (more than NK_SAMPLE_LONG points): one workgroup per cell, the points dealt round-robin, the
// partial sums joined by the fixed tree of nk_sample.h.
template <typename T, int ND>
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_sample_adjoint_long(SampleGrid g, int64_t npoints, int64_t ncells, int m,
                                                                         const int64_t* __restrict__ cell,
                                                                         const double* __restrict__ frac,
                                                                         const int64_t* __restrict__ perm,
                                                                         const int64_t* __restrict__ cell_start,
                                                                         const int64_t* __restrict__ long_cell,
                                                                         const T* __restrict__ y, double* __restrict__ acc) {
  __shared__ double s_wave[NK_SAMPLE_BLOCK / 64];
  const int64_t c = long_cell[blockIdx.x];
  if (c < 0 || c >= ncells) return;  // (the same for the whole workgroup)
  int64_t lo = cell_start[c], hi = cell_start[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > npoints ? npoints : hi;
  if (hi - lo <= NK_SAMPLE_LONG) return;
  double s = nk_sample_cell_sum<T, ND>(frac, perm, y, npoints, m, lo + threadIdx.x, hi, NK_SAMPLE_BLOCK);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = s_wave[0];
    for (int w = 1; w < NK_SAMPLE_BLOCK / 64; ++w) total += s_wave[w];
    int64_t idx[ND];
    nk_sample_decode<ND>(cell[lo], g.n, idx);
    acc[nk_sample_corner<ND>(idx, g.n, m)] += total;
  }
}

// the fp64 sums of a single-precision adjoint, rounded once
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_sample_round(int64_t n, const double* __restrict__ acc, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NK_SAMPLE_BLOCK + threadIdx.x;
  if (i < n) __builtin_nontemporal_store((float)acc[i], out + i);
}

// (o, j, i) of a flat index into an (outer, n, inner) array
__device__ __forceinline__ void regrid_split(int64_t flat, int64_t n, int64_t inner, int64_t* o, int64_t* j, int64_t* i) {
  if (flat <= 0xffffffffll && inner <= 0xffffffffll && n <= 0xffffffffll) {
    const uint32_t f = (uint32_t)flat, in = (uint32_t)inner, nn = (uint32_t)n;
    const uint32_t q = f / in;
    *i = f - q * in;
    *j = q % nn;
    *o = q / nn;
  } else {
    const int64_t q = flat / inner;
    *i = flat - q * inner;
    *j = q % n;
    *o = q / n;
  }
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_regrid_times(int64_t total, int64_t n_old, int64_t n_new, int64_t inner,
                                                                  const int64_t* __restrict__ bindex, const double* __restrict__ frac,
                                                                  const TI* __restrict__ in, TO* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * NK_SAMPLE_BLOCK + threadIdx.x;
  if (t >= total) return;
  int64_t o, j, i;
  regrid_split(t, n_new, inner, &o, &j, &i);
  int64_t b = bindex[j];
  b = b < 0 ? 0 : b > n_old - 2 ? n_old - 2 : b;
  __builtin_nontemporal_store((TO)nk_regrid_gather<TI>(in + o * n_old * inner + i, inner, b, frac[j]), out + t);
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(NK_SAMPLE_BLOCK) k_regrid_adjoint(int64_t total, int64_t n_old, int64_t n_new, int64_t inner,
                                                                    const int64_t* __restrict__ rstart, const double* __restrict__ frac,
                                                                    const TI* __restrict__ in, TO* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * NK_SAMPLE_BLOCK + threadIdx.x;
  if (t >= total) return;
  int64_t o, j, i;
  regrid_split(t, n_old, inner, &o, &j, &i);
  __builtin_nontemporal_store((TO)nk_regrid_scatter<TI>(in + o * n_new * inner + i, inner, rstart, frac, j, n_new), out + t);
}

int sample_validate(const nk_sample_plan* p, const char* what, int64_t* cells) {
  if (!p) return nk_set_error(NK_ERR_INVALID, what);
  if (p->ndim < 1 || p->ndim > 3) return nk_set_error(NK_ERR_UNSUPPORTED, "nk_sample: 1, 2 or 3 grid axes are served");
  int64_t total = 1;
  for (int a = 0; a < p->ndim; ++a) {
    if (p->n[a] < 1 || p->n[a] > 0x7fffffffLL) return nk_set_error(NK_ERR_INVALID, "nk_sample: bad axis length");
    if (total > ((int64_t)1 << 46) / p->n[a]) return nk_set_error(NK_ERR_INVALID, "nk_sample: grid too large");
    total *= p->n[a];
  }
  if (p->npoints < 0 || p->npoints > 0x7fffffffLL * NK_SAMPLE_BLOCK) return nk_set_error(NK_ERR_INVALID, "nk_sample: bad number of points");
  if (p->ncells < 0 || p->ncells > p->npoints || p->nlong < 0 || p->nlong > p->ncells || p->nlong > 0x7fffffffLL)
    return nk_set_error(NK_ERR_INVALID, "nk_sample: bad number of occupied cells");
  if (p->npoints > 0 && (!p->cell || !p->frac || !p->perm || !p->cell_start || (p->nlong > 0 && !p->long_cell)))
    return nk_set_error(NK_ERR_INVALID, "nk_sample: missing plan arrays");
  *cells = total;
  return NK_OK;
}

SampleGrid sample_grid(const nk_sample_plan* p) {
  SampleGrid g;
  for (int a = 0; a < 3; ++a) g.n[a] = a < p->ndim ? p->n[a] : 1;
  return g;
}

unsigned sample_blocks(int64_t n) { return (unsigned)((n + NK_SAMPLE_BLOCK - 1) / NK_SAMPLE_BLOCK); }

#define SAMPLE_DISPATCH(dtype, ndim, KERNEL_CALL)                                 \
  if ((dtype) == NK_F32) {                                                        \
    typedef float T;                                                              \
    if ((ndim) == 1) { constexpr int ND = 1; KERNEL_CALL; }                       \
    else if ((ndim) == 2) { constexpr int ND = 2; KERNEL_CALL; }                  \
    else { constexpr int ND = 3; KERNEL_CALL; }                                   \
  } else {                                                                        \
    typedef double T;                                                             \
    if ((ndim) == 1) { constexpr int ND = 1; KERNEL_CALL; }                       \
    else if ((ndim) == 2) { constexpr int ND = 2; KERNEL_CALL; }                  \
    else { constexpr int ND = 3; KERNEL_CALL; }                                   \
  }

#define REGRID_DISPATCH(in_dtype, out_dtype, KERNEL_CALL)                                         \
  if ((in_dtype) == NK_F32 && (out_dtype) == NK_F32) { typedef float TI; typedef float TO; KERNEL_CALL; }        \
  else if ((in_dtype) == NK_F32) { typedef float TI; typedef double TO; KERNEL_CALL; }            \
  else if ((out_dtype) == NK_F32) { typedef double TI; typedef float TO; KERNEL_CALL; }           \
  else { typedef double TI; typedef double TO; KERNEL_CALL; }

int regrid_validate(int64_t outer, int64_t n_old, int64_t n_new, int64_t inner, const void* tab, const double* frac,
                    const void* in, int in_dtype, void* out, int out_dtype, int64_t n_out, int64_t* total) {
  if ((in_dtype != NK_F32 && in_dtype != NK_F64) || (out_dtype != NK_F32 && out_dtype != NK_F64))
    return nk_set_error(NK_ERR_INVALID, "nk_regrid: dtype must be NK_F32 or NK_F64");
  if (outer < 0 || inner < 0 || n_old < 2 || n_new < 1 || n_new > n_old || n_old > 0x7fffffffLL)
    return nk_set_error(NK_ERR_INVALID, "nk_regrid: need 1 <= n_new <= n_old, n_old >= 2");
  if (!tab || !frac) return nk_set_error(NK_ERR_INVALID, "nk_regrid: missing axis tables");
  if (outer > 0 && inner > 0 && (outer > ((int64_t)1 << 46) / inner || outer * inner > ((int64_t)1 << 46) / n_old))
    return nk_set_error(NK_ERR_UNSUPPORTED, "nk_regrid: array too large for one launch");
  *total = outer * n_out * inner;
  if (*total > 0 && (!in || !out)) return nk_set_error(NK_ERR_INVALID, "nk_regrid: bad argument");
  if (*total > 0x7fffffffLL * NK_SAMPLE_BLOCK) return nk_set_error(NK_ERR_UNSUPPORTED, "nk_regrid: array too large for one launch");
  return NK_OK;
}

}  // namespace

extern "C" int nk_sample_times(const nk_sample_plan* p, const void* grid, void* pts, int dtype, void* stream) {
  int64_t cells = 0;
  int rc = sample_validate(p, "nk_sample_times: bad plan", &cells);
  if (rc != NK_OK) return rc;
  if (dtype != NK_F32 && dtype != NK_F64) return nk_set_error(NK_ERR_INVALID, "dtype must be NK_F32 or NK_F64");
  if (p->npoints == 0) return NK_OK;
  if (!grid || !pts) return nk_set_error(NK_ERR_INVALID, "nk_sample_times: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const SampleGrid g = sample_grid(p);
  SAMPLE_DISPATCH(dtype, p->ndim, {
    hipLaunchKernelGGL((k_sample_times<T, ND>), dim3(sample_blocks(p->npoints)), dim3(NK_SAMPLE_BLOCK), 0, st, g, p->npoints, p->cell,
                       p->frac, p->perm, (const T*)grid, (T*)pts);
    rc = nk_check_launch("k_sample_times");
  })
  return rc;
}

extern "C" int nk_sample_adjoint(const nk_sample_plan* p, const void* pts, void* grid, double* acc, int dtype, void* stream) {
  int64_t cells = 0;
  int rc = sample_validate(p, "nk_sample_adjoint: bad plan", &cells);
  if (rc != NK_OK) return rc;
  if (dtype != NK_F32 && dtype != NK_F64) return nk_set_error(NK_ERR_INVALID, "dtype must be NK_F32 or NK_F64");
  if (!grid || (p->npoints > 0 && !pts)) return nk_set_error(NK_ERR_INVALID, "nk_sample_adjoint: bad argument");
  if (dtype == NK_F32 && !acc) return nk_set_error(NK_ERR_INVALID, "nk_sample_adjoint: single precision needs the fp64 scratch");
  if (cells > 0x7fffffffLL * NK_SAMPLE_BLOCK) return nk_set_error(NK_ERR_UNSUPPORTED, "nk_sample_adjoint: grid too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  double* sum = dtype == NK_F32 ? acc : (double*)grid;
  hipError_t e = hipMemsetAsync(sum, 0, (size_t)cells * sizeof(double), st);
  if (e != hipSuccess) return nk_set_hip_error(e, "nk_sample_adjoint: hipMemsetAsync");
  const SampleGrid g = sample_grid(p);
  if (p->npoints > 0) {
    SAMPLE_DISPATCH(dtype, p->ndim, {
      for (int m = 0; m < (1 << ND) && rc == NK_OK; ++m) {
        hipLaunchKernelGGL((k_sample_adjoint_short<T, ND>), dim3(sample_blocks(p->ncells)), dim3(NK_SAMPLE_BLOCK), 0, st, g, p->npoints,
                           p->ncells, m, p->cell, p->frac, p->perm, p->cell_start, (const T*)pts, sum);
        rc = nk_check_launch("k_sample_adjoint_short");
        if (rc == NK_OK && p->nlong > 0) {
          hipLaunchKernelGGL((k_sample_adjoint_long<T, ND>), dim3((unsigned)p->nlong), dim3(NK_SAMPLE_BLOCK), 0, st, g, p->npoints,
                             p->ncells, m, p->cell, p->frac, p->perm, p->cell_start, p->long_cell, (const T*)pts, sum);
          rc = nk_check_launch("k_sample_adjoint_long");
        }
      }
    })
  }
  if (rc == NK_OK && dtype == NK_F32) {
    hipLaunchKernelGGL(k_sample_round, dim3(sample_blocks(cells)), dim3(NK_SAMPLE_BLOCK), 0, st, cells, (const double*)sum, (float*)grid);
    rc = nk_check_launch("k_sample_round");
  }
  return rc;
}

extern "C" int nk_regrid_times(int64_t outer, int64_t n_old, int64_t n_new, int64_t inner, const int64_t* bindex, const double* frac,
                               const void* in, int in_dtype, void* out, int out_dtype, void* stream) {
  int64_t total = 0;
  int rc = regrid_validate(outer, n_old, n_new, inner, bindex, frac, in, in_dtype, out, out_dtype, n_new, &total);
  if (rc != NK_OK || total == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  REGRID_DISPATCH(in_dtype, out_dtype, {
    hipLaunchKernelGGL((k_regrid_times<TI, TO>), dim3(sample_blocks(total)), dim3(NK_SAMPLE_BLOCK), 0, st, total, n_old, n_new, inner,
                       bindex, frac, (const TI*)in, (TO*)out);
    rc = nk_check_launch("k_regrid_times");
  })
  return rc;
}

extern "C" int nk_regrid_adjoint(int64_t outer, int64_t n_old, int64_t n_new, int64_t inner, const int64_t* rstart, const double* frac,
                                 const void* in, int in_dtype, void* out, int out_dtype, void* stream) {
  int64_t total = 0;
  int rc = regrid_validate(outer, n_old, n_new, inner, rstart, frac, in, in_dtype, out, out_dtype, n_old, &total);
  if (rc != NK_OK || total == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  REGRID_DISPATCH(in_dtype, out_dtype, {
    hipLaunchKernelGGL((k_regrid_adjoint<TI, TO>), dim3(sample_blocks(total)), dim3(NK_SAMPLE_BLOCK), 0, st, total, n_old, n_new, inner,
                       rstart, frac, (const TI*)in, (TO*)out);
    rc = nk_check_launch("k_regrid_adjoint");
  })
  return rc;
}
