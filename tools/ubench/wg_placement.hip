// Where the hardware puts the workgroups of an attention-product launch: a grid of (32, 1, 32) workgroups of 256 threads with the
// LDS footprint of gemm_tile_kernel<64, 64> (18 KB: 8 per CU), each busy for a given time; every workgroup records its XCC, shader
// engine / array / CU and its start and end time.  Prints how workgroup ids map to CUs - the assumption behind csrc/batch_plan.h
// (consecutive ids are dealt over the CUs, id and id + 256 share one) - for: all workgroups busy 20 us; the plain order of a ragged
// batch (workgroups of the padding exit at once); the same work in planned order.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/wg_placement.hip -o wg_placement && ./wg_placement
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

struct Rec { unsigned hw, xcc; unsigned long long t0, t1; };

__global__ __launch_bounds__(256) void probe(const int* __restrict__ ticks, Rec* __restrict__ out) {
  __shared__ float pad[18 * 256];
  const int id = blockIdx.z * gridDim.x + blockIdx.x;
  const unsigned long long t0 = wall_clock64();
  pad[threadIdx.x] = (float)id;
  const int want = ticks[id];                                   // 100 MHz ticks
  float acc = 0.f;
  for (int it = 0; it < 2000000 && (long long)(wall_clock64() - t0) < want; ++it) acc += pad[(threadIdx.x + it) & 255];
  if (threadIdx.x == 0) {
    Rec r;
    r.hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));           // HW_ID
    r.xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));         // XCC_ID
    r.t0 = t0; r.t1 = wall_clock64();
    out[id] = r;
    if (acc == 12345.678f) out[id].hw = 0;                      // keeps the loop
  }
}

static int cu_key(const Rec& r) { return (int)(((r.xcc & 15) << 8) | (((r.hw >> 13) & 7) << 5) | (((r.hw >> 12) & 1) << 4) | ((r.hw >> 8) & 15)); }

static void run(const char* name, const std::vector<int>& ticks_h) {
  const int n = 1024;
  int* ticks; Rec* out;
  hipMalloc(&ticks, n * sizeof(int)); hipMalloc(&out, n * sizeof(Rec));
  hipMemcpy(ticks, ticks_h.data(), n * sizeof(int), hipMemcpyHostToDevice);
  std::vector<Rec> r(n);
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(probe, dim3(32, 1, 32), dim3(256), 0, 0, ticks, out);
    if (hipDeviceSynchronize() != hipSuccess) { std::printf("launch failed\n"); return; }
  }
  hipMemcpy(r.data(), out, n * sizeof(Rec), hipMemcpyDeviceToHost);
  std::map<int, int> cu_index;
  for (const Rec& x : r) cu_index.emplace(cu_key(x), 0);
  int k = 0;
  for (auto& kv : cu_index) kv.second = k++;
  std::vector<long> load(k, 0), count(k, 0);
  int same256 = 0, same_xcc8 = 0;
  unsigned long long tmin = ~0ull, tmax = 0;
  for (int i = 0; i < n; ++i) {
    const int c = cu_index[cu_key(r[i])];
    load[c] += ticks_h[i]; count[c] += ticks_h[i] > 0;
    if (i >= 256) same256 += cu_key(r[i]) == cu_key(r[i - 256]);
    if (i >= 8) same_xcc8 += (r[i].xcc & 15) == (r[i - 8].xcc & 15);
    tmin = std::min(tmin, r[i].t0); tmax = std::max(tmax, r[i].t1);
  }
  std::printf("== %s: %d CUs seen; id and id - 8 on one XCC: %d / %d; id and id - 256 on one CU: %d / %d; span %.1f us\n", name, k, same_xcc8,
              n - 8, same256, n - 256, (double)(tmax - tmin) / 100.0);
  std::printf("   busy workgroups per CU: min %ld max %ld;  requested busy time per CU (us): min %.1f max %.1f mean %.1f\n",
              *std::min_element(count.begin(), count.end()), *std::max_element(count.begin(), count.end()),
              *std::min_element(load.begin(), load.end()) / 100.0, *std::max_element(load.begin(), load.end()) / 100.0,
              [&] { long s = 0; for (long v : load) s += v; return (double)s / k / 100.0; }());
  std::printf("   first 40 ids -> xcc.se.sh.cu:");
  for (int i = 0; i < 40; ++i) std::printf(" %u.%u.%u.%u", r[i].xcc & 15, (r[i].hw >> 13) & 7, (r[i].hw >> 12) & 1, (r[i].hw >> 8) & 15);
  std::printf("\n   ids 256..271:");
  for (int i = 256; i < 272; ++i) std::printf(" %u.%u.%u.%u", r[i].xcc & 15, (r[i].hw >> 13) & 7, (r[i].hw >> 12) & 1, (r[i].hw >> 8) & 15);
  std::printf("\n");
  hipFree(ticks); hipFree(out);
}

int main() {
  const int src[16] = {128, 123, 117, 115, 113, 112, 111, 96, 83, 82, 82, 81, 78, 63, 60, 55};      // the canonical batch, x 8 frames
  std::vector<int> all(1024, 2000), plain(1024, 0), planned(1024, 0);
  std::vector<int> work;                                                                              // per active tile, 0.5 us per K-block
  for (int z = 0; z < 32; ++z) {
    const int L = 8 * src[z / 2], blocks = (L + 31) / 32;
    for (int t = 0; t < 32; ++t)
      if ((t / 2) * 64 < L) { plain[z * 32 + t] = 50 * blocks; work.push_back(50 * blocks); }
  }
  std::sort(work.begin(), work.end(), [](int a, int b) { return a > b; });
  const int na = (int)work.size();
  for (int p = 0; p < na; ++p) {
    const int layer = p / 256, r = p % 256, width = std::min(256, na - layer * 256);
    planned[layer * 256 + ((layer & 1) ? width - 1 - r : r)] = work[p];
  }
  run("all busy 20 us", all);
  run("ragged batch, plain order", plain);
  run("ragged batch, planned order", planned);
  return 0;
}
