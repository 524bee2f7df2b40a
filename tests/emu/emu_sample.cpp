// TEST-ONLY host emulation of the sampling kernels (nifty_amd/csrc/nk_sample.hip): the same per-element bodies
// (nk_sample.h), run thread after thread and pass after pass in the kernels' launch order.  tests/test_sampling_ops.py
// compiles this file on its own and holds it to the bounds of the device tests.  Never linked into the product library.
#define NK_HOST_EMU 1
#include <vector>

#include "../../nifty_amd/csrc/nk_sample.h"

namespace {

template <typename T, int ND>
void times(const int64_t* n, int64_t npoints, const int64_t* cell, const double* frac, const int64_t* perm, const T* x, T* y) {
  for (int64_t k = 0; k < npoints; ++k) {  // thread k of k_sample_times
    double e[ND];
    for (int a = 0; a < ND; ++a) e[a] = frac[k * ND + a];
    const double acc = nk_sample_gather<T, ND>(n, cell[k], e, x);
    const int64_t o = perm[k];
    if ((uint64_t)o < (uint64_t)npoints) y[o] = (T)acc;
  }
}

template <typename T, int ND>
void adjoint(const int64_t* n, int64_t npoints, int64_t ncells, const int64_t* cell, const double* frac, const int64_t* perm,
             const int64_t* cell_start, int64_t nlong, const int64_t* long_cell, const T* y, T* out) {
  int64_t size = 1;
  for (int a = 0; a < ND; ++a) size *= n[a];
  std::vector<double> acc(size, 0.0);  // the memset
  for (int m = 0; m < (1 << ND); ++m) {
    for (int64_t c = 0; c < ncells; ++c) {  // thread c of k_sample_adjoint_short
      const int64_t lo = cell_start[c], hi = cell_start[c + 1];
      if (hi <= lo || hi - lo > NK_SAMPLE_LONG) continue;
      const double s = nk_sample_cell_sum<T, ND>(frac, perm, y, npoints, m, lo, hi, 1);
      int64_t idx[ND];
      nk_sample_decode<ND>(cell[lo], n, idx);
      acc[nk_sample_corner<ND>(idx, n, m)] += s;
    }
    for (int64_t b = 0; b < nlong; ++b) {  // workgroup b of k_sample_adjoint_long
      const int64_t c = long_cell[b];
      const int64_t lo = cell_start[c], hi = cell_start[c + 1];
      if (hi - lo <= NK_SAMPLE_LONG) continue;
      double part[NK_SAMPLE_BLOCK];
      for (int t = 0; t < NK_SAMPLE_BLOCK; ++t)
        part[t] = nk_sample_cell_sum<T, ND>(frac, perm, y, npoints, m, lo + t, hi, NK_SAMPLE_BLOCK);
      const double total = nk_sample_tree_host(part);
      int64_t idx[ND];
      nk_sample_decode<ND>(cell[lo], n, idx);
      acc[nk_sample_corner<ND>(idx, n, m)] += total;
    }
  }
  for (int64_t i = 0; i < size; ++i) out[i] = (T)acc[i];  // fp64: acc IS the output; fp32: k_sample_round
}

template <typename TI, typename TO>
void regrid(int adj, int64_t outer, int64_t n_old, int64_t n_new, int64_t inner, const int64_t* table, const double* frac,
            const TI* in, TO* out) {
  const int64_t n_in = adj ? n_new : n_old, n_out = adj ? n_old : n_new;
  for (int64_t t = 0; t < outer * n_out * inner; ++t) {  // thread t of k_regrid_times / k_regrid_adjoint
    const int64_t q = t / inner, i = t - q * inner, j = q % n_out, o = q / n_out;
    const TI* col = in + o * n_in * inner + i;
    out[t] = adj ? (TO)nk_regrid_scatter<TI>(col, inner, table, frac, j, n_new)
                 : (TO)nk_regrid_gather<TI>(col, inner, table[j], frac[j]);
  }
}

}  // namespace

#define EMU_DISPATCH(CALL)                                    \
  if (dtype == 0) {                                           \
    typedef float T;                                          \
    if (ndim == 1) { constexpr int ND = 1; CALL; }            \
    else if (ndim == 2) { constexpr int ND = 2; CALL; }       \
    else if (ndim == 3) { constexpr int ND = 3; CALL; }       \
    else return -1;                                           \
  } else {                                                    \
    typedef double T;                                         \
    if (ndim == 1) { constexpr int ND = 1; CALL; }            \
    else if (ndim == 2) { constexpr int ND = 2; CALL; }       \
    else if (ndim == 3) { constexpr int ND = 3; CALL; }       \
    else return -1;                                           \
  }

// dtype 0: float32, 1: float64 (NK_F32 / NK_F64)
extern "C" int emu_sample_times(int ndim, const int64_t* n, int64_t npoints, const int64_t* cell, const double* frac,
                                const int64_t* perm, const void* x, void* y, int dtype) {
  EMU_DISPATCH((times<T, ND>(n, npoints, cell, frac, perm, (const T*)x, (T*)y)))
  return 0;
}

extern "C" int emu_sample_adjoint(int ndim, const int64_t* n, int64_t npoints, int64_t ncells, const int64_t* cell,
                                  const double* frac, const int64_t* perm, const int64_t* cell_start, int64_t nlong,
                                  const int64_t* long_cell, const void* y, void* out, int dtype) {
  EMU_DISPATCH((adjoint<T, ND>(n, npoints, ncells, cell, frac, perm, cell_start, nlong, long_cell, (const T*)y, (T*)out)))
  return 0;
}

extern "C" int emu_regrid(int adj, int64_t outer, int64_t n_old, int64_t n_new, int64_t inner, const int64_t* table,
                          const double* frac, const void* in, int in_dtype, void* out, int out_dtype) {
  if (in_dtype == 0 && out_dtype == 0) regrid<float, float>(adj, outer, n_old, n_new, inner, table, frac, (const float*)in, (float*)out);
  else if (in_dtype == 0) regrid<float, double>(adj, outer, n_old, n_new, inner, table, frac, (const float*)in, (double*)out);
  else if (out_dtype == 0) regrid<double, float>(adj, outer, n_old, n_new, inner, table, frac, (const double*)in, (float*)out);
  else regrid<double, double>(adj, outer, n_old, n_new, inner, table, frac, (const double*)in, (double*)out);
  return 0;
}
