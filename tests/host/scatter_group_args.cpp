// Host-side argument checks of nk_octant_scatter_k2_group, as a stand-alone program for a sanitizer build (no device call is
// reached: every case is refused before the first launch, so it runs on a machine without a GPU):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tests/host/scatter_group_args.cpp \
//         nifty_amd/csrc/nk_vec.hip nifty_amd/csrc/nk_util.hip -o build/scatter_group_args && build/scatter_group_args
//
// The pointer tables hold addresses that are never dereferenced on the host; tables shorter than four entries make an
// out-of-range read of the checks themselves (n above the limit, entries past n) an AddressSanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "niftyk.h"

static int failures = 0;

static void expect(const char* what, int rc, int want, const char* text) {
  const char* msg = nk_last_error();
  const bool ok = rc == want && (!text || (msg && std::strstr(msg, text)));
  std::printf("%-34s rc=%d (%s)%s\n", what, rc, msg ? msg : "", ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
}

int main() {
  static double cell[10];  // stand-ins for device arrays: distinct addresses, never read through
  const int64_t shape[3] = {16, 16, 256}, huge[3] = {8192, 8192, 8192}, four[4] = {4, 4, 4, 4};
  const int32_t* pidx = reinterpret_cast<const int32_t*>(&cell[6]);
  const int32_t* k2 = reinterpret_cast<const int32_t*>(&cell[7]);
  const double* w8[2] = {&cell[0], &cell[0]};  // one array as two members is allowed
  const double* wmax[2] = {&cell[1], &cell[2]};
  double* scratch[2] = {&cell[3], &cell[4]};
  double* abar[2] = {&cell[8], &cell[9]};
  const double* w8_null[2] = {&cell[0], nullptr};
  double* same[2] = {&cell[3], &cell[3]};
  const int64_t nb = 4720;

  expect("n = 0", nk_octant_scatter_k2_group(3, shape, 0, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "1 <= n <= 4");
  expect("n = 5", nk_octant_scatter_k2_group(3, shape, 5, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "1 <= n <= 4");
  expect("n = -1", nk_octant_scatter_k2_group(3, shape, -1, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "1 <= n <= 4");
  expect("ndim 0", nk_octant_scatter_k2_group(0, shape, 2, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, nullptr);
  expect("ndim 4", nk_octant_scatter_k2_group(4, four, 2, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, nullptr);
  expect("null shape", nk_octant_scatter_k2_group(3, nullptr, 2, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, nullptr);
  expect("null w8 table", nk_octant_scatter_k2_group(3, shape, 2, nullptr, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("null pidx", nk_octant_scatter_k2_group(3, shape, 2, w8, nullptr, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("null bin_k2", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, nullptr, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("null scratch table", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, nb, nullptr, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("null abar table", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, nb, scratch, nullptr, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("nb = 0", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, 0, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("nb = 2^31", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, (int64_t)1 << 31, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "bad argument");
  expect("null member w8", nk_octant_scatter_k2_group(3, shape, 2, w8_null, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_INVALID, "null member");
  expect("members share a scratch", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, nb, same, abar, wmax, nullptr), NK_ERR_INVALID, "share");
  expect("members share an output", nk_octant_scatter_k2_group(3, shape, 2, w8, pidx, k2, nb, scratch, same, wmax, nullptr), NK_ERR_INVALID, "share");
  expect("k^2 range too large", nk_octant_scatter_k2_group(3, huge, 2, w8, pidx, k2, nb, scratch, abar, wmax, nullptr), NK_ERR_UNSUPPORTED, "k^2 range too large");
  expect("k^2 range, no scales", nk_octant_scatter_k2_group(3, huge, 2, w8, pidx, k2, nb, scratch, abar, nullptr, nullptr), NK_ERR_UNSUPPORTED, "k^2 range too large");
  std::printf("%s\n", failures ? "FAILED" : "scatter_group_args OK");
  return failures ? 1 : 0;
}
