// Binding of the amplitude staging kernel (hea_amp.hip).  The launch goes on torch's current HIP stream (composes
// with hipGraph capture); extents are checked here against what the kernel will index, so a short buffer is a Python
// exception, never a GPU fault.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

extern "C" int qfx_hea_amp_stage(const float* x, long F, long ld, int S, int n, uint32_t* psi, float scale, int bf16,
                                 hipStream_t st);

namespace {

void need(bool ok, const std::string& msg) {
  if (!ok) throw std::invalid_argument("hea_amp_stage: " + msg);
}

// x [S, F <= 2^n] fp32, unit inner stride, any row stride ld >= F -> psi [S * 2^n] int32 words (re, 0) in fp16 or
// bf16: x / ||x||_2 (float64 norm; a zero row -> the uniform state) times ``scale`` (a power of two), rounded once
void hea_amp_stage(torch::Tensor x, int64_t n, torch::Tensor psi, double scale, bool bf16) {
  need(x.defined() && x.is_cuda() && x.scalar_type() == torch::kFloat32, "x must be a float32 CUDA tensor");
  need(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1, "x must be [S, F] with S, F >= 1");
  const int64_t S = x.size(0), F = x.size(1);
  need(x.stride(1) == 1, "x needs unit inner stride");
  const int64_t ld = S > 1 ? x.stride(0) : F;
  need(n >= 8 && n <= 30, "8..30 qubits");
  need(F <= (int64_t(1) << n), "more features than amplitudes (F > 2^n)");
  need(ld >= F, "row stride below the row length");
  need(S <= INT32_MAX, "too many samples");
  // the rows lie inside x's storage
  const int64_t avail = (int64_t)(x.storage().nbytes() / sizeof(float)) - x.storage_offset();
  need((S - 1) * ld + F <= avail, "rows reach past x's storage");
  need(psi.defined() && psi.is_cuda() && psi.is_contiguous() && psi.scalar_type() == torch::kInt32,
       "psi must be a contiguous int32 CUDA tensor");
  need(psi.get_device() == x.get_device(), "x and psi on different devices");
  need(psi.numel() >= (S << n), "psi too small (" + std::to_string(psi.numel()) + " < " + std::to_string(S << n) + ")");
  need((reinterpret_cast<uintptr_t>(psi.data_ptr()) & 15) == 0, "psi must be 16-byte aligned");
  int e = 0;
  need(scale > 0 && std::frexp(scale, &e) == 0.5, "scale must be a power of two");
  const int rc = qfx_hea_amp_stage(x.data_ptr<float>(), (long)F, (long)ld, (int)S, (int)n,
                                   reinterpret_cast<uint32_t*>(psi.data_ptr()), (float)scale, bf16 ? 1 : 0,
                                   c10::hip::getCurrentHIPStream().stream());
  if (rc != 0) throw std::runtime_error("qfx_hea_amp_stage failed: " + std::to_string(rc));
}

}  // namespace

void register_hea_amp(pybind11::module& m) {
  m.def("hea_amp_stage", &hea_amp_stage, pybind11::arg("x"), pybind11::arg("n"), pybind11::arg("psi"),
        pybind11::arg("scale"), pybind11::arg("bf16") = false);
}
