// ptnn_dims.hpp -- the row lengths and strides that follow from a topology (n_in, n_hidden, n_out): ONE set of formulas for the
// host (ptnn_create fills the handle with them, ptnn_host.hpp) and for the device (a kernel with the hidden width compiled in
// forms them at compile time, ptnn_dev_pack.hpp: PackDims).  plan_launch checks the two against each other before it picks such
// a kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace ptnn {

__host__ __device__ constexpr int round_up4(int v) { return (v + 3) & ~3; }
__host__ __device__ constexpr int dims_P(int I, int H, int O) { return I * H + H * O + H + O; }      // parameters of the net
__host__ __device__ constexpr int dims_PS(int P) { return round_up4(P + 1); }                        // state row: (w, eta), whole float4s
__host__ __device__ constexpr int dims_PW(int P) { return (P + 15) & ~15; }                          // pos_w trace row: whole 64-byte sectors
__host__ __device__ constexpr int dims_IPY(int I) { return round_up4(I + 2); }                       // data row: x[I], y, then 1 + x[n].x[n-1] for the pipelined SGD epoch
__host__ __device__ constexpr int dims_FWS(int I, int O) { return round_up4(I + 1 + O); }            // packed forward row of one hidden unit

}  // namespace ptnn
