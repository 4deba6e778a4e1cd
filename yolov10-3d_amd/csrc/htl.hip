// Hierarchical task learning (GUPNet): the per-epoch weights of the 12 loss items, kept and updated on the device.
//
// Reference: utils/htl.py:23-56 Hierarchical_Task_Learning.compute_weight, as engine/trainer.py:357-358 calls it at every epoch start.
// One launch of one workgroup restates it on device state, in fp32 and in the reference's operation order.  Nothing is read back and the
// weight table keeps its address, so the loss kernels (y3d_loss3d_weighted) read the table that the last update left.
//
//   htl.py:26-32   items without predecessors (box, cls) start at 1, the others at 0
//   htl.py:34-38   only when the list already holds stat_epochs entries: mean_diff = mean(past[:-2] - past[2:]) over the stat_epochs - 2
//                  differences; init_diff = the first mean_diff ever computed
//   htl.py:39      c = 1 - relu(mean_diff / init_diff); torch's relu keeps NaN (fmaxf(NaN, 0) is 0 and would hide it)
//   htl.py:41-47   w = time_value ** (1 - prod(c[predecessors])), the product starting from 1.0; powf(0, 0) = 1, powf(0, < 0) = inf
//   htl.py:53-54   the oldest entry is dropped, and the current loss is appended AFTER the weights were computed
//   htl.py:56      w / sum(w) * 6
#include "common.h"

namespace {

constexpr int HTL_N = 12;

// utils/htl.py:8-21 loss_graph, as indices into the 12 items (one-to-many set first); -1 = none
__device__ __forceinline__ void htl_pre(int j, int& p0, int& p1) {
  const int base = j < 6 ? 0 : 6, k = j - base;
  p0 = k >= 2 ? base : -1;          // dep, o3d, s3d, hd <- box
  p1 = k == 2 ? base + 4 : -1;      // dep <- s3d as well
}

__global__ __launch_bounds__(64) void htl_update_kernel(const float* __restrict__ items, float time_value, int S, float* __restrict__ ring,
                                                        int* __restrict__ count, float* __restrict__ init_diff, int* __restrict__ have_init,
                                                        float* __restrict__ weights, int* __restrict__ status) {
  __shared__ float sc[HTL_N], sw[HTL_N];
  const int j = threadIdx.x;
  int n = count[0];
  n = n < 0 ? 0 : (n > S ? S : n);  // a corrupt count never indexes outside the ring
  const bool full = n == S;
  int p0 = -1, p1 = -1;
  if (j < HTL_N) htl_pre(j, p0, p1);
  float w = p0 < 0 ? 1.f : 0.f;
  float cur = 0.f;
  if (j < HTL_N) {
    cur = items[j];
    if (full) {
      float s = 0.f;
      for (int i = 0; i + 2 < S; ++i) s += ring[i * HTL_N + j] - ring[(i + 2) * HTL_N + j];
      const float md = s / (float)(S - 2);
      float id = init_diff[j];
      if (!have_init[0]) { id = md; init_diff[j] = md; }
      const float r = md / id;
      sc[j] = 1.f - (r > 0.f ? r : (r != r ? r : 0.f));
    }
  }
  __syncthreads();
  if (j < HTL_N) {
    if (full) {
      if (p0 >= 0) {
        float cw = 1.0f;
        cw *= sc[p0];
        if (p1 >= 0) cw *= sc[p1];
        w = powf(time_value, 1.f - cw);
      }
      for (int i = 0; i + 1 < S; ++i) ring[i * HTL_N + j] = ring[(i + 1) * HTL_N + j];  // htl.py:53 pop(0): each lane moves its own column
      ring[(S - 1) * HTL_N + j] = cur;
    } else {
      ring[n * HTL_N + j] = cur;
    }
    sw[j] = w;
  }
  __syncthreads();
  if (j < HTL_N) {
    float sum = 0.f;
    for (int i = 0; i < HTL_N; ++i) sum += sw[i];
    const float o = w / sum * 6.0f;
    weights[j] = o;
    if (!(fabsf(o) <= 3.4028234663852886e38f) || !(fabsf(sum) <= 3.4028234663852886e38f)) atomicOr(status, 1);
  }
  if (j == 0) {
    if (full) have_init[0] = 1;
    else count[0] = n + 1;
  }
}

}  // namespace

extern "C" int y3d_htl_update(const float* items, float time_value, int stat_epochs, float* ring, int* count, float* init_diff, int* have_init,
                              float* weights, int* status, void* stream) {
  Y3D_CHECK(items && ring && count && init_diff && have_init && weights && status, "htl_update: NULL pointer");
  Y3D_CHECK(stat_epochs >= 3 && stat_epochs <= 8, "htl_update: stat_epochs in 3..8 (got %d)", stat_epochs);
  hipLaunchKernelGGL(htl_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, items, time_value, stat_epochs, ring, count, init_diff,
                     have_init, weights, status);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}
