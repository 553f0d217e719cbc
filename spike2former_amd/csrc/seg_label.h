// What segmetric.hip (scoring) and segdraw.hip (drawing) agree on about ONE value of a label map: which class it is.
#pragma once
#include <stdint.h>

// -> the class index in [0, K), or -1: the value is no class
__device__ __forceinline__ int pred_class(int64_t p, int K) { return (p >= 0 && p < (int64_t)K) ? (int)p : -1; }
// a float map counts where it holds a class index exactly (the 0 / 1 maps of a one-class head); NaN fails every comparison
__device__ __forceinline__ int pred_class(float p, int K) { return (p >= 0.0f && p < (float)K && p == truncf(p)) ? (int)p : -1; }

// LoadAnnotations(reduce_zero_label=True) on the raw annotation
__device__ __forceinline__ int64_t seg_reduce_zero_label(int64_t l) { return (l == 0 || l == 255) ? 255 : l - 1; }

// f(PredT(), LabelT()) for the (checked) dtype codes
template <class F>
int seg_by_types(int pred_dtype, int label_dtype, const F& f) {
  if (pred_dtype == S2F_SEG_PRED_I64) return label_dtype == S2F_SEG_LABEL_U8 ? f(int64_t(), uint8_t()) : f(int64_t(), int64_t());
  return label_dtype == S2F_SEG_LABEL_U8 ? f(float(), uint8_t()) : f(float(), int64_t());
}
