// enf_grad_chunked.h -- what the chunked gradient / VJP (enf_grad_chunked.hip) needs of the one-launch path
// (enf_grad.hip): whether a flow fits one gradient launch, and the single-launch calls a chunk runs through.
#pragma once
#include "enf_train.h"

namespace enf {

inline enf_status hip_status(hipError_t e) {
  return e == hipSuccess ? ENF_OK : set_error(ENF_ERR_HIP, hipGetErrorString(e));
}

// Is the flow within one gradient launch's bounds (<= 16 layers, <= 32 steps, accumulators and activations in LDS)?
bool fits_one_launch(bool f64, int64_t D, int64_t N, const enf_layer* layers, int32_t nlayers);
// The rest: a flow that fits one launch (N >= 1 for single_workspace)
enf_status single_workspace(bool f64, int64_t D, int64_t N, const enf_layer* layers, int32_t nlayers, size_t* bytes);
enf_status negll_grad_single(bool f64, int64_t D, int64_t N, const void* X, int64_t ldx, const enf_layer* layers,
                             int32_t nlayers, void* out, void* workspace, size_t workspace_bytes, hipStream_t st);
enf_status flow_vjp_single(bool f64, int64_t D, int64_t N, const void* X, int64_t ldx, const void* dY, int64_t lddy,
                           const void* dladj, const enf_layer* layers, int32_t nlayers, void* dX, int64_t lddx,
                           void* dparams, void* workspace, size_t workspace_bytes, hipStream_t st);
// B: the global batch size the update normalises by (N on one rank); ar: the cross-rank sum between the gradient
// and the update (enf_whitening_step_dp), or none; nranks: the ranks of that sum.
enf_status whitening_step_single(bool f64, int64_t D, int64_t N, const void* X, int64_t ldx, const enf_layer* layers,
                                 int32_t nlayers, void* theta, void* acc, const int64_t* runs, int32_t nruns,
                                 const int64_t* hb, int32_t nhb, double eta, double epsilon, double* loss_out,
                                 void* workspace, size_t workspace_bytes, hipStream_t st, int64_t B, AllreduceFn ar,
                                 void* ar_ctx, int nranks);

}  // namespace enf
