// Per-step segmentation metrics from ONE pass over (argmax predictions, targets): a CxC confusion
// matrix built in LDS, then accuracy / Jaccard / F-beta derived on the device (no host sync).
//
// Replaces the four torchmetrics 0.7.3 updates of reference vision_mtl/lit_module.py:48-69,106-118
// (Accuracy average="micro"; FBetaScore beta=1 average="weighted" mdmc_average="global";
// JaccardIndex absent_score=0, mean over classes).  torchmetrics is not installable offline, so
// the formulas are restated from its documented definitions ("parity unpinned").
//
// The *_ex entry points take torchmetrics' ignore_index: a pixel whose TARGET equals it is not counted.  When it names a
// class in [0, C), that class has an empty row (zero support in F-beta by construction) and is left out of the Jaccard
// class mean (divide by C - 1); predictions of it on valid pixels stay in their true class's row, so they still count
// against that class and in the accuracy, which is over the valid pixels.
#include "common.h"

#define CM_MAX_C 64

// IGN: skip the pixels whose target is `ignore` (the plain instantiation never reads it)
template <bool IGN>
__global__ __launch_bounds__(256) void confusion_kernel(const long long* __restrict__ pred,
                                                        const long long* __restrict__ tgt, int* __restrict__ cm,
                                                        long long P, int C, long long ignore) {
  extern __shared__ int hist[];
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  VMTL_GRID_STRIDE(i, P) {
    const long long t = tgt[i], p = pred[i];
    if ((!IGN || t != ignore) && t >= 0 && t < C && p >= 0 && p < C) atomicAdd(&hist[(int)t * C + (int)p], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += blockDim.x)
    if (hist[i]) atomicAdd(&cm[i], hist[i]);  // integer atomics: exact and order independent
}

// out[0] accuracy (micro), out[1] Jaccard (mean over classes, absent -> 0), out[2] F-beta (support-weighted).
// Class `ign` (-1: none) is left out of the Jaccard mean; its row of cm is empty, so accuracy and F-beta need no change.
__global__ void segm_metrics_kernel(const int* __restrict__ cm, int C, float beta, float* out, int ign) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double total = 0.0, correct = 0.0, jac = 0.0, fb = 0.0, support_sum = 0.0;
  const double b2 = (double)beta * beta;
  for (int c = 0; c < C; ++c) {
    double tp = cm[c * C + c], row = 0.0, col = 0.0;
    for (int k = 0; k < C; ++k) {
      row += cm[c * C + k];  // targets of class c
      col += cm[k * C + c];  // predictions of class c
    }
    const double fn = row - tp, fp = col - tp;
    total += row;
    correct += tp;
    const double uni = tp + fp + fn;
    if (c != ign) jac += uni > 0.0 ? tp / uni : 0.0;
    const double den = (1.0 + b2) * tp + b2 * fn + fp;
    fb += row * (den > 0.0 ? (1.0 + b2) * tp / den : 0.0);
    support_sum += row;
  }
  const int nc = ign >= 0 ? C - 1 : C;
  out[0] = (float)(total > 0.0 ? correct / total : 0.0);
  out[1] = (float)(nc > 0 ? jac / nc : 0.0);
  out[2] = (float)(support_sum > 0.0 ? fb / support_sum : 0.0);
}

template <bool IGN>
static int confusion_launch(const long long* pred, const long long* target, int* cm, long long P, int C,
                            long long ignore, void* stream) {
  if (!pred || !target || !cm || P <= 0 || C <= 0 || C > CM_MAX_C) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cm, 0, (size_t)C * C * sizeof(int), st) != hipSuccess) return VMTL_ERR_LAUNCH;
  hipLaunchKernelGGL(confusion_kernel<IGN>, dim3(grid_1d(P, 256 * 8, 1024)), dim3(256), (size_t)C * C * sizeof(int), st, pred,
                     target, cm, P, C, ignore);
  return vmtl_check_launch();
}

// ign: the class left out of the Jaccard mean, -1 for none
static int segm_metrics_launch(const int* cm, int C, float beta, int ign, float* out, void* stream) {
  if (!cm || !out || C <= 0 || C > CM_MAX_C) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(segm_metrics_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cm, C, beta, out, ign);
  return vmtl_check_launch();
}

extern "C" int vmtl_confusion_matrix(const long long* pred, const long long* target, int* cm, long long P, int C,
                                     void* stream) {
  VMTL_ENTER();
  return confusion_launch<false>(pred, target, cm, P, C, 0, stream);
}

extern "C" int vmtl_confusion_matrix_ex(const long long* pred, const long long* target, int* cm, long long P, int C,
                                        long long ignore_index, void* stream) {
  VMTL_ENTER();
  return confusion_launch<true>(pred, target, cm, P, C, ignore_index, stream);
}

extern "C" int vmtl_segm_metrics(const int* cm, int C, float beta, float* out, void* stream) {
  VMTL_ENTER();
  return segm_metrics_launch(cm, C, beta, -1, out, stream);
}

// cm as vmtl_confusion_matrix_ex(..., ignore_index) built it
extern "C" int vmtl_segm_metrics_ex(const int* cm, int C, float beta, long long ignore_index, float* out, void* stream) {
  VMTL_ENTER();
  return segm_metrics_launch(cm, C, beta, ignore_index >= 0 && ignore_index < C ? (int)ignore_index : -1, out, stream);
}
