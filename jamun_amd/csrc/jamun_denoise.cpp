// jamun_denoise.cpp — the C entries of the denoising evaluation (jamun_denoise.hip): jamun_noise_align_graphs and jamun_denoise_loss.  They
// touch no jamun_sampler: the forward between them is jamun_xhat.  Every refusal is raised before any launch; the checks that need no HIP
// call come first, so a caller without a GPU sees them.
#include <cmath>

#include "jamun_host.h"

namespace {

// 3 n_atoms, and a loop index one stride past it, fit an int
constexpr int32_t kMaxAtoms = (INT32_MAX - 65536) / 3;

void check_batch(int32_t n_graphs, int32_t n_atoms, float sigma) {
  if (n_graphs < 0 || n_atoms < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
  if (!std::isfinite(sigma) || !(sigma > 0.f)) throw Err(JAMUN_ERR_INVALID, "sigma " + std::to_string(sigma) + " must be finite and above 0");
  if (n_atoms > kMaxAtoms) throw Err(JAMUN_ERR_INVALID, "n_atoms " + std::to_string(n_atoms) + ": 3 n_atoms must fit 31 bits");
  if (n_graphs == INT32_MAX) throw Err(JAMUN_ERR_INVALID, "n_graphs + 1 must fit 31 bits");
}

// the kernels read the table on the device: a host pointer would fault there
void require_device_table(const int32_t* ptr_dev) {
  hipPointerAttribute_t attr{};
  const hipError_t e = hipPointerGetAttributes(&attr, ptr_dev);
  if (e != hipSuccess) (void)hipGetLastError();  // (an address the runtime does not know: not an error of the stream)
  if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && !attr.isManaged)) throw Err(JAMUN_ERR_INVALID, "ptr_dev is not device memory");
}

}  // namespace

extern "C" {

int jamun_noise_align_graphs(const float* x_dev, const float* noise_dev, const int32_t* ptr_dev, int32_t n_graphs, int32_t n_atoms, float sigma,
                             int32_t mean_center, int32_t align, float* x_c_dev, float* y_dev, float* rmsd_dev, void* stream) {
  return guarded([&] {
    if (!x_dev || !noise_dev || !ptr_dev || !x_c_dev || !y_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    check_batch(n_graphs, n_atoms, sigma);
    if (n_graphs == 0) return;
    require_device_table(ptr_dev);
    launch_noise_align(x_dev, noise_dev, ptr_dev, n_graphs, n_atoms, sigma, mean_center != 0, align != 0, x_c_dev, y_dev, rmsd_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_denoise_loss(const float* xhat_dev, const float* x_c_dev, const int32_t* ptr_dev, int32_t n_graphs, int32_t n_atoms, float sigma,
                       const float* loss_weight_dev, float inv_c_out_sq, float* out_dev, void* stream) {
  return guarded([&] {
    if (!xhat_dev || !x_c_dev || !ptr_dev || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    check_batch(n_graphs, n_atoms, sigma);
    if (n_graphs == 0) return;
    require_device_table(ptr_dev);
    const float rmsd_scale = sigma * 1.7320508075688772f;  // sigma * np.sqrt(D) in fp32 (denoiser.py:271)
    launch_denoise_loss(xhat_dev, x_c_dev, ptr_dev, n_graphs, n_atoms, rmsd_scale, loss_weight_dev, inv_c_out_sq, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

}  // extern "C"
