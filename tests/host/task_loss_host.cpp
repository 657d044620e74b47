// The element math of nt_task_loss (notorch_amd/csrc/task_loss_math.hpp) on the host, for
// tests/test_task_loss_host.py: reads batches from stdin, writes results to stdout, loads nothing else of
// the project.  Little-endian, packed.  Build by hand:
//   g++ -std=c++17 -O2 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tests/host/task_loss_host.cpp -o task_loss_host
//
// A batch is a 28-byte header { int32 kind, int32 c, int32 dtype, float v_kl, float eps, int64 n } and n records;
// batches follow each other until the end of the input.
//   kind = NT_LOSS_MSE .. NT_LOSS_XENT, dtype = NT_F32 / NT_BF16 (P = float / uint16_t):
//     record: P preds[c], float target, uint8 lt, uint8 gt
//     result: float L, P grad[c]            task_loss_element<kind, P>(preds, target, c, v_kl, eps, lt, gt, 1, grad)
//   kind = 100: record float x,   result float    digammaf(x)
//   kind = 101: record float x,   result uint16   float_to_bf16_bits(x)
//   kind = 102: record uint16 u,  result float    bf16_bits_to_float(u)
// Exit status 0; 2 on a malformed input (a message goes to stderr).
#include "../../notorch_amd/csrc/task_loss_math.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

enum { kDigamma = 100, kToBf16 = 101, kFromBf16 = 102 };

struct Header {
  int32_t kind, c, dtype;
  float v_kl, eps;
  int64_t n;
};
constexpr size_t kHeaderBytes = 28;

bool read_all(void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }
bool write_all(const void* src, size_t bytes) { return bytes == 0 || fwrite(src, 1, bytes, stdout) == bytes; }

template <int KIND, typename P>
bool run_elements(const Header& h) {
  const size_t c = (size_t)h.c, rec = c * sizeof(P) + 6, res = 4 + c * sizeof(P);
  std::vector<unsigned char> in((size_t)h.n * rec), out((size_t)h.n * res);
  if (!read_all(in.data(), in.size())) return false;
  std::vector<P> p(c), g(c);
  for (int64_t e = 0; e < h.n; ++e) {
    const unsigned char* r = in.data() + (size_t)e * rec;
    float y;
    memcpy(p.data(), r, c * sizeof(P));
    memcpy(&y, r + c * sizeof(P), 4);
    const bool lt = r[c * sizeof(P) + 4] != 0, gt = r[c * sizeof(P) + 5] != 0;
    const float L = nt::task_loss_element<KIND, P>(p.data(), y, h.c, h.v_kl, h.eps, lt, gt, 1.f, g.data());
    unsigned char* o = out.data() + (size_t)e * res;
    memcpy(o, &L, 4);
    memcpy(o + 4, g.data(), c * sizeof(P));
  }
  return write_all(out.data(), out.size());
}

template <typename P>
bool run_kind(const Header& h) {
  switch (h.kind) {
    case NT_LOSS_MSE: return run_elements<NT_LOSS_MSE, P>(h);
    case NT_LOSS_MAE: return run_elements<NT_LOSS_MAE, P>(h);
    case NT_LOSS_RMSE: return run_elements<NT_LOSS_RMSE, P>(h);
    case NT_LOSS_BCE: return run_elements<NT_LOSS_BCE, P>(h);
    case NT_LOSS_MVE: return run_elements<NT_LOSS_MVE, P>(h);
    case NT_LOSS_EVIDENTIAL: return run_elements<NT_LOSS_EVIDENTIAL, P>(h);
    default: return run_elements<NT_LOSS_XENT, P>(h);
  }
}

template <typename In, typename Out, typename F>
bool run_map(const Header& h, F f) {
  std::vector<In> in((size_t)h.n);
  std::vector<Out> out((size_t)h.n);
  if (!read_all(in.data(), in.size() * sizeof(In))) return false;
  for (size_t i = 0; i < in.size(); ++i) out[i] = f(in[i]);
  return write_all(out.data(), out.size() * sizeof(Out));
}

int fail(const char* what) {
  fprintf(stderr, "task_loss_host: %s\n", what);
  return 2;
}

}  // namespace

int main() {
  for (;;) {
    unsigned char raw[kHeaderBytes];
    const size_t got = fread(raw, 1, kHeaderBytes, stdin);
    if (got == 0) break;
    if (got != kHeaderBytes) return fail("truncated header");
    Header h;
    memcpy(&h.kind, raw, 4), memcpy(&h.c, raw + 4, 4), memcpy(&h.dtype, raw + 8, 4);
    memcpy(&h.v_kl, raw + 12, 4), memcpy(&h.eps, raw + 16, 4), memcpy(&h.n, raw + 20, 8);
    if (h.n < 0 || h.n > ((int64_t)1 << 28)) return fail("bad record count");
    bool ok;
    if (h.kind == kDigamma) {
      ok = run_map<float, float>(h, [](float x) { return nt::digammaf(x); });
    } else if (h.kind == kToBf16) {
      ok = run_map<float, uint16_t>(h, [](float x) { return nt::float_to_bf16_bits(x); });
    } else if (h.kind == kFromBf16) {
      ok = run_map<uint16_t, float>(h, [](uint16_t u) { return nt::bf16_bits_to_float(u); });
    } else {
      if (h.kind < NT_LOSS_MSE || h.kind > NT_LOSS_XENT) return fail("unknown kind");
      if (h.dtype != NT_F32 && h.dtype != NT_BF16) return fail("unknown dtype");
      const int want_c = h.kind == NT_LOSS_MVE ? 2 : h.kind == NT_LOSS_EVIDENTIAL ? 4 : h.kind == NT_LOSS_XENT ? h.c : 1;
      if (h.c < 1 || h.c > (1 << 20) || h.c != want_c) return fail("c does not fit the kind");
      ok = h.dtype == NT_F32 ? run_kind<float>(h) : run_kind<uint16_t>(h);
    }
    if (!ok) return fail("truncated records or a failed write");
  }
  return fflush(stdout) == 0 ? 0 : 2;
}
