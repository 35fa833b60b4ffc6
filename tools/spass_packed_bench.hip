// spass_packed_bench.hip — go / no-go of the packed S stream: k_spass_sup on plain tiles against the same
// kernel on the exact 58-bit packed copy (csrc/riptrm_spack.h), same box, same process, alternated.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<pkg>/csrc -Iinclude tools/spass_packed_bench.hip \
//   <pkg>/csrc/riptrm_{si,stiefel,trs,trs_big,grassmann,grassmann_so}.hip -ldl -o spass_packed_bench
// (riptrm_kernels.hip is included below and brings the C-ABI, which refers to the other translation units).
// Usage: spass_packed_bench [n = 4000] [instances = 64] [rounds = 12] [launches per round = 10]
// Random S (sum of four uniforms, scaled like N(0, 2/n)), one right-hand side per instance, every
// instance active: the launch the headline solve repeats.  Both variants run the whole kernel, burst-
// buffered partial stores included, and must leave the same bits in the partial grid.  Prints one
// JSON line: us per launch (median / min / max over the rounds) and TB/s of PLAIN-EQUIVALENT bytes
// (the plain layout's bytes over the time) for both, plus the bytes the packed variant really reads.
#include "riptrm_kernels.hip"
#include <algorithm>

using namespace riptrm;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

__global__ void k_fill(double* p, int64_t count, uint64_t seed, double scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + seed;
    double s = -2.0;
    for (int k = 0; k < 4; ++k) {   // splitmix64
      z += 0x9E3779B97F4A7C15ull;
      uint64_t x = z;
      x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
      x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
      x ^= x >> 31;
      s += (double)(x >> 11) * 0x1.0p-53;
    }
    p[i] = s * scale;
  }
}

static double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 4000, B = argc > 2 ? atoi(argv[2]) : 64;
  const int rounds = argc > 3 ? atoi(argv[3]) : 12, per = argc > 4 ? atoi(argv[4]) : 10;
  if (n < 2 || B < 1 || B > 65535 || rounds < 1 || per < 1) return 2;
  const Layout L = make_layout(n, B, 0, RIPTRM_LAYOUT_SYMTILE);
  const int64_t stride = s_elems_of(n, RIPTRM_LAYOUT_SYMTILE), nfull = spk_nfull_of(n);
  int ncu = 256;
  CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  double* S;
  char *ws, *spk;
  int32_t* word;
  CK(hipMalloc(&S, (size_t)B * stride * 8));
  CK(hipMalloc(&ws, (size_t)L.total));
  CK(hipMalloc(&spk, (size_t)B * std::max<int64_t>(nfull, 1) * SPK_TILE_BYTES));
  CK(hipMalloc(&word, (size_t)B * std::max<int64_t>(nfull, 1) * 4));
  CK(hipMemset(ws, 0, (size_t)L.total));
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, S, (int64_t)B * stride, 1ull, sqrt(2.0 / n) * 1.7320508);
  hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, (double*)(ws + L.off_vec), (int64_t)NVEC * B * L.ld, 2ull, 1.0);
  CK(hipGetLastError());

  DevParams P;
  std::memset(&P, 0, sizeof(P));
  P.S = S; P.inst_stride = stride; P.ld = L.ld; P.n = n; P.batch = B; P.layout = RIPTRM_LAYOUT_SYMTILE;
  P.nt = L.nt; P.ntiles = (int)ntiles_of(n); P.wl = edge_w_of(n); P.nst = nst_of(n); P.nsup = (int32_t)nsup_of(n);
  P.smode = 1; P.pbuf = (double*)(ws + L.off_pbuf); P.pbatch = B; P.vec = (double*)(ws + L.off_vec);
  P.lists = (int32_t*)(ws + L.off_lists); P.cnt = (int32_t*)(ws + L.off_cnt);
  P.spk_ntf = spk_ntf_of(n); P.spk_nfull = (int32_t)nfull; P.spk_stride = nfull * SPK_TILE_BYTES;
  hipLaunchKernelGGL(k_list_range, dim3((B + 255) / 256), dim3(256), 0, 0, P, 0, B);
  if (nfull > 0) hipLaunchKernelGGL(k_spack<false>, dim3((unsigned)nfull, (unsigned)B), dim3(SP_THREADS), 0, 0, P, spk, word, (unsigned long long*)nullptr);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<int32_t> hw((size_t)B * nfull);
  CK(hipMemcpy(hw.data(), word, hw.size() * 4, hipMemcpyDeviceToHost));
  int64_t packed = 0;
  for (int32_t x : hw) packed += x != 0;

  DevParams V[2] = {P, P};   // 0: plain (no packed copy), 1: packed
  V[0].spk_ntf = V[0].spk_nfull = 0; V[0].spk_stride = 0;
  V[1].spk = spk; V[1].spk_word = word;
  const int64_t units = (int64_t)B * P.nsup;
  const unsigned grid = (unsigned)(units < ncu ? units : ncu);
  const size_t pbytes = (size_t)B * pgrid_of(n) * 8;
  std::vector<double> out[2] = {std::vector<double>(pbytes / 8), std::vector<double>(pbytes / 8)};
  for (int v = 0; v < 2; ++v) {   // warm-up + the result of each variant
    CK(hipMemset(P.pbuf, 0, pbytes));
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(k_spass_sup, dim3(grid), dim3(SP_THREADS), 0, 0, V[v], 0, -1);
    CK(hipGetLastError());
    CK(hipMemcpy(out[v].data(), P.pbuf, pbytes, hipMemcpyDeviceToHost));
  }
  const bool same = std::memcmp(out[0].data(), out[1].data(), pbytes) == 0;

  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  std::vector<float> us[2];
  for (int r = 0; r < rounds; ++r)
    for (int v = 0; v < 2; ++v) {
      CK(hipEventRecord(a, 0));
      for (int k = 0; k < per; ++k) hipLaunchKernelGGL(k_spass_sup, dim3(grid), dim3(SP_THREADS), 0, 0, V[v], 0, -1);
      CK(hipEventRecord(b, 0));
      CK(hipEventSynchronize(b));
      CK(hipGetLastError());
      float ms = 0;
      CK(hipEventElapsedTime(&ms, a, b));
      us[v].push_back(ms * 1e3f / per);
    }
  const double plain_bytes = (double)B * stride * 8;
  const double real_bytes = plain_bytes - (double)packed * ((double)TS * TS * 8 - SPK_TILE_BYTES);
  printf("{\"tool\": \"spass_packed_bench\", \"n\": %d, \"instances\": %d, \"grid\": %u, \"rounds\": %d, \"launches_per_round\": %d, "
         "\"full_tiles\": %lld, \"tiles_packed\": %lld, \"results_bitwise_equal\": %s, \"plain_bytes\": %.0f, \"packed_bytes\": %.0f",
         n, B, grid, rounds, per, (long long)(B * nfull), (long long)packed, same ? "true" : "false", plain_bytes, real_bytes);
  for (int v = 0; v < 2; ++v) {
    const double med = median(us[v]), lo = *std::min_element(us[v].begin(), us[v].end()), hi = *std::max_element(us[v].begin(), us[v].end());
    printf(", \"%s\": {\"us_median\": %.2f, \"us_min\": %.2f, \"us_max\": %.2f, \"plain_equiv_TBps_median\": %.3f, \"bus_TBps_median\": %.3f}",
           v ? "packed" : "plain", med, lo, hi, plain_bytes / med * 1e-6, (v ? real_bytes : plain_bytes) / med * 1e-6);
  }
  printf("}\n");
  return same ? 0 : 1;
}
