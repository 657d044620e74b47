// notorch_amd/csrc/dirichlet_math.hpp on the host, for tests/test_dirichlet_host.py.  stdin: int32 what, int32 k,
// float v_kl, int32 n, then n records; stdout: n results (little-endian fp32).
//   what = 0: record logits[k], target;  result L, grad[k]    dirichlet_element<float>(..., s = 1, grad)
//   what = 1: record x;                  result trigammaf(x)
//   g++ -std=c++17 -O2 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tests/host/dirichlet_host.cpp -o dirichlet_host
#include "../../notorch_amd/csrc/dirichlet_math.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

int main() {
  int32_t head[4];
  if (fread(head, 4, 4, stdin) != 4) return 2;
  float v_kl;
  memcpy(&v_kl, &head[2], 4);
  const int what = head[0], k = head[1], n = head[3];
  if (what < 0 || what > 1 || k < 1 || n < 0) return 2;
  const size_t rec = what == 1 ? 1 : (size_t)k + 1;
  std::vector<float> io((size_t)n * rec), g((size_t)k);
  if (fread(io.data(), 4, io.size(), stdin) != io.size()) return 2;
  for (int e = 0; e < n; ++e) {
    float* r = io.data() + (size_t)e * rec;
    if (what == 1) {
      r[0] = nt::trigammaf(r[0]);
    } else {
      r[0] = nt::dirichlet_element<float>(r, r[k], k, v_kl, 1.f, g.data());  // reads r before it is overwritten
      memcpy(r + 1, g.data(), (size_t)k * 4);
    }
  }
  return fwrite(io.data(), 4, io.size(), stdout) == io.size() && fflush(stdout) == 0 ? 0 : 2;
}
