// Host-side declarations shared between the kernel files of libouniverse (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "ou_kernels.h"

namespace ou {
// per-family set-up (dynamic LDS limits); called once from init_conv_kernels()
hipError_t init_chain_kernels();
hipError_t init_direct3_kernels();
hipError_t init_block3_kernels();
hipError_t init_direct4_kernels();
hipError_t init_split_kernels();

// One conv launch, decided but not enqueued.  Every plan_* function is pure host code: no stream, no HIP call;
// asking "would this family take the layer" is reading `status` of its plan.
struct ConvPlan {
  hipError_t status;  // hipSuccess; hipErrorInvalidConfiguration = "not a layer for this family"; hipErrorNotSupported = "not with
                      // this fused epilogue" (fused FIR, activating store: the caller's fallback); hipErrorInvalidValue
  int variant;        // the code cfg_out receives (ou_variants.h)
  void (*kern)(ConvArgs);
  dim3 grid, block;
  size_t smem;
  ConvArgs args;      // the filled-in copy the kernel receives
};
inline ConvPlan no_plan(hipError_t why) { return ConvPlan{why, -1, nullptr, dim3(), dim3(), 0, ConvArgs()}; }
// the launch site of every void (*)(ConvArgs) kernel: p.status when there is nothing to launch, else the launch error
hipError_t launch_plan(const ConvPlan& p, hipStream_t stream);
// the whole dispatch behind launch_conv(): the families below in kConvFamilies' order, then the LDS-tiled configs
ConvPlan plan_conv(const ConvArgs& a, int num_cu);
ConvPlan plan_conv_direct(const ConvArgs& a, int num_cu);
ConvPlan plan_conv_direct3(const ConvArgs& a, int num_cu);
ConvPlan plan_conv_direct4(const ConvArgs& a, int num_cu);
// the 401-frame levels at small batch: conv_direct4_kernel picks its tile height for an even fill of the CUs there
inline bool direct4_short_layer(const ConvArgs& a) { return a.Nq < 1024 && a.B < 4; }
ConvPlan plan_conv_direct4w(const ConvArgs& a, int num_cu);
// the bf16-split form of the stride-1 k3 / k5 convs (conv_split_kernel)
ConvPlan plan_conv_split(const ConvArgs& a, int num_cu);
// Small-K rate-change convs of the wide levels (what they compute: beside launch_conv in ou_kernels.h); hipErrorNotSupported =
// not a shape for them.  (num_cu: unused, one signature for every plan function)
ConvPlan plan_rate_down(const ConvArgs& a, int num_cu = 0);
ConvPlan plan_rate_up(const ConvArgs& a, int num_cu = 0);
}  // namespace ou
