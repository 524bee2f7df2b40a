// nk_nufft.hip -- the non-uniform FFT of Nufft / Gridder (nifty_amd/nufft.py; include/niftyk.h "non-uniform FFT").
//
// TIMES  = spread (type 1) -> nk_fftn(inverse = 1) -> nk_nufft_crop      points -> real grid
// ADJOINT = nk_nufft_pad -> nk_fftn(inverse = 0) -> interpolate (type 2)  real grid -> points
//
// Exponential-of-semicircle kernel phi(z) = exp(beta (sqrt(1 - (2 z / w)^2) - 1)) of width w <= 16 on the oversampled grid;
// a point at u (grid units, [0, n)) covers the cells l0 .. l0 + w - 1, l0 = ceil(u - w / 2), wrapped modulo n.  The host
// builds the plan (nifty_amd.nufft.NufftPlan): the points sorted by TILE of the oversampled grid, the bin offsets, the work
// items of the spreading pass and the correction tables.  No float atomics anywhere: every output is summed by one thread
// (or one fixed lane tree) in an order that depends on the plan only, so results are bit-reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nk_util.h"

namespace {

constexpr int NU_CELLS = 256;    // cells of one tile = threads of a spreading workgroup
constexpr int NU_BATCH = 64;     // points staged in LDS per step of the spreading walk
constexpr int NU_WMAX = 16;      // widest kernel: register arrays and LDS rows are sized for it
constexpr int NU_MAXNB = 512;    // neighbour bins one tile may visit (at most 7 x 7 x 7 = 343)
constexpr int NU_LANES = 16;     // lanes that share one point in the interpolation

template <typename T>
struct NuVec;
template <>
struct NuVec<float> {
  typedef float2 type;
};
template <>
struct NuVec<double> {
  typedef double2 type;
};

__device__ __forceinline__ float nu_es(float z, float beta, float two_over_w) {
  const float x = z * two_over_w;
  const float r = 1.0f - x * x;
  return expf(beta * (sqrtf(r > 0.0f ? r : 0.0f) - 1.0f));
}
__device__ __forceinline__ double nu_es(double z, double beta, double two_over_w) {
  const double x = z * two_over_w;
  const double r = 1.0 - x * x;
  return exp(beta * (sqrt(r > 0.0 ? r : 0.0) - 1.0));
}

// first cell of a point's footprint (unwrapped, may be negative) and the offset z of that cell from the point
__device__ __forceinline__ int nu_first_cell(double u, int w, double* z0) {
  const double l = ceil(u - 0.5 * w);
  *z0 = l - u;
  return (int)l;
}

// Spreading: ONE workgroup per work item = (tile of the oversampled grid, chunk of the tile's point list).  A tile's list is
// the concatenation, in a fixed order, of the points of every bin within `reach` bins of it (wrapping); each thread owns one
// cell of the tile and adds, point by point in list order, the point's value times the product of its separable kernel
// values (staged in LDS per batch) when the cell lies in the point's footprint.  The sum goes straight into the grid (slab
// < 0: the item is the whole list, zeros included) or into slab `slab` of the scratch (a split list, summed by
// k_nufft_slab_sum in chunk order).
template <typename T, int ND>
__global__ void __launch_bounds__(NU_CELLS) k_nufft_spread(nk_nufft_plan p, const T* __restrict__ pts, T* __restrict__ grid,
                                                          double* __restrict__ slab) {
  __shared__ int64_t s_first[NU_MAXNB];
  __shared__ int64_t s_cum[NU_MAXNB + 1];
  __shared__ T s_ker[NU_BATCH][ND][NU_WMAX];
  __shared__ double s_z0[NU_BATCH][ND];
  __shared__ int s_l0[NU_BATCH][ND];
  __shared__ T s_v[NU_BATCH][2];
  __shared__ int s_hit[NU_BATCH];

  const int tid = threadIdx.x;
  const int64_t* it = p.item + 4 * (int64_t)blockIdx.x;
  const int64_t tile = it[0], lo = it[1], hi = it[2], sl = it[3];
  const int w = p.w;
  int tc[3], vis[3], b0[3];
  int64_t rem = tile;
  for (int d = ND - 1; d >= 0; --d) {
    tc[d] = (int)(rem % p.ntiles[d]);
    rem /= p.ntiles[d];
  }
  int nb = 1;
  for (int d = 0; d < ND; ++d) {
    const int span = 2 * p.reach[d] + 1;
    vis[d] = span < p.ntiles[d] ? span : p.ntiles[d];
    b0[d] = span < p.ntiles[d] ? (tc[d] - p.reach[d] + p.ntiles[d]) % p.ntiles[d] : 0;
    nb *= vis[d];
  }
  for (int k = tid; k < nb; k += NU_CELLS) {
    int r = k, o[3];
    for (int d = ND - 1; d >= 0; --d) {
      o[d] = r % vis[d];
      r /= vis[d];
    }
    int64_t b = 0;
    for (int d = 0; d < ND; ++d) b = b * p.ntiles[d] + (b0[d] + o[d]) % p.ntiles[d];
    s_first[k] = p.bin_start[b];
    s_cum[k + 1] = p.bin_start[b + 1] - p.bin_start[b];
  }
  __syncthreads();
  if (tid == 0) {
    s_cum[0] = 0;
    for (int k = 0; k < nb; ++k) s_cum[k + 1] += s_cum[k];
  }
  __syncthreads();

  int c[3], ts[3];
  bool valid = true;
  {
    int r = tid;
    for (int d = ND - 1; d >= 0; --d) {
      ts[d] = tc[d] * p.tile[d];
      c[d] = ts[d] + r % p.tile[d];
      r /= p.tile[d];
      valid = valid && c[d] < p.n[d];
    }
  }
  const T beta = (T)p.beta, two_over_w = (T)(2.0 / w);
  double acc_re = 0.0, acc_im = 0.0;
  for (int64_t base = lo; base < hi; base += NU_BATCH) {
    const int cnt = (int)(hi - base < NU_BATCH ? hi - base : NU_BATCH);
    if (tid < cnt) {
      const int64_t pos = base + tid;
      int kl = 0, kh = nb - 1;  // the neighbour bin holding list position pos
      while (kl < kh) {
        const int mid = (kl + kh + 1) >> 1;
        if (s_cum[mid] <= pos) kl = mid;
        else kh = mid - 1;
      }
      const int64_t s = s_first[kl] + (pos - s_cum[kl]);
      const int64_t orig = p.perm[s];
      s_v[tid][0] = pts[2 * orig];
      s_v[tid][1] = pts[2 * orig + 1];
      bool hit = true;
      for (int d = 0; d < ND; ++d) {
        double z0;
        int l0 = nu_first_cell(p.u[s * ND + d], w, &z0);
        if (l0 < 0) l0 += p.n[d];
        s_z0[tid][d] = z0;
        s_l0[tid][d] = l0;
        // footprint [l0, l0 + w) and tile [ts, ts + tile) meet (cyclically)
        const int a = ts[d] - l0, b = l0 - ts[d];
        hit = hit && ((a < 0 ? a + p.n[d] : a) < w || (b < 0 ? b + p.n[d] : b) < p.tile[d]);
      }
      s_hit[tid] = hit;
    }
    __syncthreads();
    for (int e = tid; e < cnt * ND * NU_WMAX; e += NU_CELLS) {
      const int q = e / (ND * NU_WMAX), d = (e / NU_WMAX) % ND, t = e % NU_WMAX;
      s_ker[q][d][t] = t < w ? nu_es((T)(s_z0[q][d] + t), beta, two_over_w) : (T)0;
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      if (!s_hit[q]) continue;  // the same for the whole workgroup
      T k = (T)1;
      bool in = true;
      for (int d = 0; d < ND; ++d) {
        int dd = c[d] - s_l0[q][d];
        dd += dd < 0 ? p.n[d] : 0;
        in = in && dd < w;
        k *= s_ker[q][d][dd < NU_WMAX ? dd : NU_WMAX - 1];
      }
      if (in) {
        acc_re += (double)(k * s_v[q][0]);
        acc_im += (double)(k * s_v[q][1]);
      }
    }
    __syncthreads();
  }
  if (sl >= 0) {
    slab[2 * (sl * NU_CELLS + tid)] = acc_re;
    slab[2 * (sl * NU_CELLS + tid) + 1] = acc_im;
  } else if (valid) {
    int64_t cell = 0;
    for (int d = 0; d < ND; ++d) cell = cell * p.n[d] + c[d];
    grid[2 * cell] = (T)acc_re;
    grid[2 * cell + 1] = (T)acc_im;
  }
}

// The tiles whose lists were split: the slabs of tile split_tile[k] are split_slab[k] .. split_slab[k + 1] - 1, added in
// that (chunk) order by the thread that owns the cell.
template <typename T, int ND>
__global__ void __launch_bounds__(NU_CELLS) k_nufft_slab_sum(nk_nufft_plan p, T* __restrict__ grid, const double* __restrict__ slab) {
  const int tid = threadIdx.x;
  int64_t rem = p.split_tile[blockIdx.x];
  int c[3];
  bool valid = true;
  int r = tid;
  for (int d = ND - 1; d >= 0; --d) {
    const int tcd = (int)(rem % p.ntiles[d]);
    rem /= p.ntiles[d];
    c[d] = tcd * p.tile[d] + r % p.tile[d];
    r /= p.tile[d];
    valid = valid && c[d] < p.n[d];
  }
  if (!valid) return;
  double re = 0.0, im = 0.0;
  for (int64_t s = p.split_slab[blockIdx.x]; s < p.split_slab[blockIdx.x + 1]; ++s) {
    re += slab[2 * (s * NU_CELLS + tid)];
    im += slab[2 * (s * NU_CELLS + tid) + 1];
  }
  int64_t cell = 0;
  for (int d = 0; d < ND; ++d) cell = cell * p.n[d] + c[d];
  grid[2 * cell] = (T)re;
  grid[2 * cell + 1] = (T)im;
}

// Interpolation: NU_LANES lanes per point, points in sorted (tile) order.  Lane t evaluates the kernel at tap t of every
// axis; the last axis is summed along a row by one lane, the rows (taps of the other axes) are dealt to the lanes
// round-robin, and the lanes are joined by a fixed xor tree.  The result goes to the point's original index.
template <typename T, int ND>
__global__ void __launch_bounds__(256) k_nufft_interp(nk_nufft_plan p, const T* __restrict__ grid, T* __restrict__ pts) {
  typedef typename NuVec<T>::type V;
  const V* g = reinterpret_cast<const V*>(grid);
  const int lane = threadIdx.x & (NU_LANES - 1);
  const int64_t s_raw = (int64_t)blockIdx.x * (256 / NU_LANES) + (threadIdx.x / NU_LANES);
  const bool live = s_raw < p.m;
  const int64_t s = live ? s_raw : p.m - 1;
  const int w = p.w;
  const T beta = (T)p.beta, two_over_w = (T)(2.0 / w);
  int l0[3];
  T ker[3];
  for (int d = 0; d < ND; ++d) {
    double z0;
    int l = nu_first_cell(p.u[s * ND + d], w, &z0);
    l0[d] = l < 0 ? l + p.n[d] : l;
    ker[d] = lane < w ? nu_es((T)(z0 + lane), beta, two_over_w) : (T)0;
  }
  double acc_re = 0.0, acc_im = 0.0;
  if (ND == 1) {
    if (lane < w) {
      int i = l0[0] + lane;
      i -= i >= p.n[0] ? p.n[0] : 0;
      const V v = g[i];
      acc_re = (double)(ker[0] * v.x);
      acc_im = (double)(ker[0] * v.y);
    }
  } else {
    T kl[NU_WMAX];  // the last axis' kernel values of every tap
#pragma unroll
    for (int t = 0; t < NU_WMAX; ++t) kl[t] = __shfl(ker[ND - 1], t, NU_LANES);
    const int nrows = ND == 2 ? w : w * w;
    const int nlast = p.n[ND - 1];
    for (int r0 = 0; r0 < nrows; r0 += NU_LANES) {
      const int r = r0 + lane;
      const int rc = r < nrows ? r : 0;
      const int t0 = ND == 2 ? rc : rc / w, t1 = ND == 2 ? 0 : rc % w;
      T krow = __shfl(ker[0], t0, NU_LANES);
      if (ND == 3) krow *= __shfl(ker[1], t1, NU_LANES);
      if (r < nrows) {
        int i0 = l0[0] + t0;
        i0 -= i0 >= p.n[0] ? p.n[0] : 0;
        int64_t row = i0;
        if (ND == 3) {
          int i1 = l0[1] + t1;
          i1 -= i1 >= p.n[1] ? p.n[1] : 0;
          row = row * p.n[1] + i1;
        }
        const V* line = g + row * nlast;
        int il = l0[ND - 1];
#pragma unroll
        for (int t = 0; t < NU_WMAX; ++t) {
          if (t < w) {
            const V v = line[il];
            const T k = krow * kl[t];
            acc_re += (double)(k * v.x);
            acc_im += (double)(k * v.y);
            il = il + 1 == nlast ? 0 : il + 1;
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = NU_LANES / 2; off > 0; off >>= 1) {
    acc_re += __shfl_xor(acc_re, off, NU_LANES);
    acc_im += __shfl_xor(acc_im, off, NU_LANES);
  }
  if (live && lane == 0) {
    const int64_t o = p.perm[s];
    pts[2 * o] = (T)acc_re;
    pts[2 * o + 1] = (T)acc_im;
  }
}

// TIMES, after the transform: out[i] = Re grid[k mod n] * corr_0[i_0] * ..., k_d = i_d - nmodes_d / 2
template <typename T, int ND>
__global__ void __launch_bounds__(256) k_nufft_crop(nk_nufft_plan p, const T* __restrict__ grid, T* __restrict__ out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int64_t rem = i, cell = 0;
  double corr = 1.0;
  int off = 0;
  int id[3];
  for (int d = ND - 1; d >= 0; --d) {
    id[d] = (int)(rem % p.nmodes[d]);
    rem /= p.nmodes[d];
  }
  for (int d = 0; d < ND; ++d) {
    int k = id[d] - p.nmodes[d] / 2;
    k += k < 0 ? p.n[d] : 0;
    cell = cell * p.n[d] + k;
    corr *= p.corr[off + id[d]];
    off += p.nmodes[d];
  }
  out[i] = (T)((double)grid[2 * cell] * corr);
}

// ADJOINT, before the transform: every cell of the oversampled grid, the corrected mode or zero
template <typename T, int ND>
__global__ void __launch_bounds__(256) k_nufft_pad(nk_nufft_plan p, const T* __restrict__ in, int in_complex, T* __restrict__ grid,
                                                   int64_t total) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= total) return;
  int64_t rem = l, idx = 0;
  int ld[3];
  for (int d = ND - 1; d >= 0; --d) {
    ld[d] = (int)(rem % p.n[d]);
    rem /= p.n[d];
  }
  bool inside = true;
  double corr = 1.0;
  int off = 0;
  for (int d = 0; d < ND; ++d) {
    const int nm = p.nmodes[d], half = nm / 2;
    int k = ld[d] < nm - half ? ld[d] : ld[d] >= p.n[d] - half ? ld[d] - p.n[d] : p.n[d];
    inside = inside && k != p.n[d];
    const int i = inside ? k + half : 0;
    idx = idx * nm + i;
    corr *= p.corr[off + i];
    off += nm;
  }
  T re = (T)0, im = (T)0;
  if (inside) {
    re = (T)((double)(in_complex ? in[2 * idx] : in[idx]) * corr);
    im = in_complex ? (T)((double)in[2 * idx + 1] * corr) : (T)0;
  }
  grid[2 * l] = re;
  grid[2 * l + 1] = im;
}

int64_t nu_prod(const int32_t* a, int nd) {
  int64_t r = 1;
  for (int d = 0; d < nd; ++d) r *= a[d];
  return r;
}

int nu_validate(const nk_nufft_plan* p, const char* what) {
  if (!p) return nk_set_error(NK_ERR_INVALID, what);
  if (p->ndim < 1 || p->ndim > 3) return nk_set_error(NK_ERR_INVALID, "nk_nufft: ndim must be 1, 2 or 3");
  if (p->w < 2 || p->w > NU_WMAX) return nk_set_error(NK_ERR_INVALID, "nk_nufft: kernel width must be 2 .. 16");
  if (p->m < 0 || p->m > 0x7fffffffLL * (256 / NU_LANES)) return nk_set_error(NK_ERR_INVALID, "nk_nufft: bad number of points");
  int64_t cells = 1, nb = 1;
  for (int d = 0; d < p->ndim; ++d) {
    if (p->nmodes[d] < 1 || p->n[d] < 2 * p->w || p->n[d] < p->nmodes[d] || p->n[d] > (1 << 30))
      return nk_set_error(NK_ERR_INVALID, "nk_nufft: oversampled length must be >= max(2 w, grid length)");
    if (p->tile[d] < 1 || p->ntiles[d] != (p->n[d] + p->tile[d] - 1) / p->tile[d] || p->reach[d] < 0)
      return nk_set_error(NK_ERR_INVALID, "nk_nufft: tile geometry does not match the oversampled grid");
    const int span = 2 * p->reach[d] + 1;
    nb *= span < p->ntiles[d] ? span : p->ntiles[d];
    cells *= p->tile[d];
  }
  if (cells != NU_CELLS) return nk_set_error(NK_ERR_INVALID, "nk_nufft: a tile must hold 256 cells");
  if (nb > NU_MAXNB) return nk_set_error(NK_ERR_INVALID, "nk_nufft: a tile visits more than 512 bins");
  if (!p->corr) return nk_set_error(NK_ERR_INVALID, "nk_nufft: missing correction table");
  if (p->m > 0 && (!p->u || !p->perm)) return nk_set_error(NK_ERR_INVALID, "nk_nufft: missing point arrays");
  return NK_OK;
}

#define NU_DISPATCH(dtype, ndim, KERNEL_CALL)                                                   \
  if ((dtype) == NK_F32) {                                                                      \
    typedef float T;                                                                            \
    if ((ndim) == 1) { constexpr int ND = 1; KERNEL_CALL; }                                     \
    else if ((ndim) == 2) { constexpr int ND = 2; KERNEL_CALL; }                                \
    else { constexpr int ND = 3; KERNEL_CALL; }                                                 \
  } else if ((dtype) == NK_F64) {                                                               \
    typedef double T;                                                                           \
    if ((ndim) == 1) { constexpr int ND = 1; KERNEL_CALL; }                                     \
    else if ((ndim) == 2) { constexpr int ND = 2; KERNEL_CALL; }                                \
    else { constexpr int ND = 3; KERNEL_CALL; }                                                 \
  } else {                                                                                      \
    return nk_set_error(NK_ERR_INVALID, "dtype must be NK_F32 or NK_F64");                      \
  }

}  // namespace

extern "C" int nk_nufft_spread(const nk_nufft_plan* p, const void* pts, void* grid, double* slab, int dtype, void* stream) {
  int rc = nu_validate(p, "nk_nufft_spread: bad plan");
  if (rc != NK_OK) return rc;
  if (p->n_items < 1 || p->n_items > 0x7fffffffLL || !p->item || !p->bin_start || !grid || (p->m > 0 && !pts))
    return nk_set_error(NK_ERR_INVALID, "nk_nufft_spread: bad argument");
  if (p->n_split < 0 || p->n_split > 0x7fffffffLL || (p->n_split > 0 && (!slab || !p->split_tile || !p->split_slab)))
    return nk_set_error(NK_ERR_INVALID, "nk_nufft_spread: split lists need the slab scratch");
  hipStream_t st = (hipStream_t)stream;
  NU_DISPATCH(dtype, p->ndim, {
    hipLaunchKernelGGL((k_nufft_spread<T, ND>), dim3((unsigned)p->n_items), dim3(NU_CELLS), 0, st, *p, (const T*)pts, (T*)grid, slab);
    rc = nk_check_launch("k_nufft_spread");
    if (rc == NK_OK && p->n_split > 0) {
      hipLaunchKernelGGL((k_nufft_slab_sum<T, ND>), dim3((unsigned)p->n_split), dim3(NU_CELLS), 0, st, *p, (T*)grid,
                         (const double*)slab);
      rc = nk_check_launch("k_nufft_slab_sum");
    }
  })
  return rc;
}

extern "C" int nk_nufft_interp(const nk_nufft_plan* p, const void* grid, void* pts, int dtype, void* stream) {
  int rc = nu_validate(p, "nk_nufft_interp: bad plan");
  if (rc != NK_OK) return rc;
  if (p->m == 0) return NK_OK;
  if (!grid || !pts) return nk_set_error(NK_ERR_INVALID, "nk_nufft_interp: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (p->m + (256 / NU_LANES) - 1) / (256 / NU_LANES);
  NU_DISPATCH(dtype, p->ndim, {
    hipLaunchKernelGGL((k_nufft_interp<T, ND>), dim3((unsigned)blocks), dim3(256), 0, st, *p, (const T*)grid, (T*)pts);
    rc = nk_check_launch("k_nufft_interp");
  })
  return rc;
}

extern "C" int nk_nufft_crop(const nk_nufft_plan* p, const void* grid, void* out, int dtype, void* stream) {
  int rc = nu_validate(p, "nk_nufft_crop: bad plan");
  if (rc != NK_OK) return rc;
  if (!grid || !out) return nk_set_error(NK_ERR_INVALID, "nk_nufft_crop: bad argument");
  const int64_t total = nu_prod(p->nmodes, p->ndim);
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return nk_set_error(NK_ERR_UNSUPPORTED, "nk_nufft_crop: grid too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  NU_DISPATCH(dtype, p->ndim, {
    hipLaunchKernelGGL((k_nufft_crop<T, ND>), dim3((unsigned)blocks), dim3(256), 0, st, *p, (const T*)grid, (T*)out, total);
    rc = nk_check_launch("k_nufft_crop");
  })
  return rc;
}

extern "C" int nk_nufft_pad(const nk_nufft_plan* p, const void* in, int in_complex, void* grid, int dtype, void* stream) {
  int rc = nu_validate(p, "nk_nufft_pad: bad plan");
  if (rc != NK_OK) return rc;
  if (!in || !grid) return nk_set_error(NK_ERR_INVALID, "nk_nufft_pad: bad argument");
  const int64_t total = nu_prod(p->n, p->ndim);
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return nk_set_error(NK_ERR_UNSUPPORTED, "nk_nufft_pad: grid too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  NU_DISPATCH(dtype, p->ndim, {
    hipLaunchKernelGGL((k_nufft_pad<T, ND>), dim3((unsigned)blocks), dim3(256), 0, st, *p, (const T*)in, in_complex ? 1 : 0,
                       (T*)grid, total);
    rc = nk_check_launch("k_nufft_pad");
  })
  return rc;
}
