// ptnn_shapes.hpp -- the compiled (task, n_in, n_out) shapes and the per-shape table of the sampler's kernels.
// Every shape is its own translation unit (ptnn_shape.hip with -DPTNN_T/-DPTNN_I/-DPTNN_O), so that the build can compile them
// in parallel; ptnn.hip only references the tables (ptnn_checkpoint.hip: through the handle).  The per-shape analysis kernels are not here: AnalysisShape (ptnn_analysis_device.hpp).
// Every fixed-width packed kernel (PTNN_PACK_FIXED, PTNN_PACKM_FIXED below) is one more translation unit of ptnn_shape.hip, with -DPTNN_HC on top.
//
// REG: the shipped time series have 4 lag inputs (REG:916); 5 and 32 cover BASELINE.json's literal [5,H,1] and the synthetic
// [32,H,1].  CLS: the reference's problem table (CLS:909-995): iris 4/3, ionosphere 34/2, cancer 9/2, wine 11/10, bank 20/2,
// pendigit 16/10, chess 6/18.  n_hidden is a run-time value in every kernel but the fixed-width packed ones: PTNN_PACK_FIXED
// lists, per shape, the hidden widths X(task, n_in, n_out, n_hidden) whose one-CU packed kernel is compiled a second time with the
// width as a literal (the reference runs every one of its time-series problems at 5 hidden units: REG:916).  A shape without an
// entry compiles no such kernel.  Each entry is a code object of its own: a kernel added to a shape's code object moves the
// addresses and the LDS kernel ids of the shape's other kernels, and those are held to their bytes (compare_device_code.py).
#pragma once
#include "ptnn_device.hpp"

#ifndef PTNN_SHAPES
#define PTNN_SHAPES(X) X(0, 4, 1) X(0, 5, 1) X(0, 32, 1) X(1, 4, 3) X(1, 34, 2) X(1, 9, 2) X(1, 11, 10) X(1, 20, 2) X(1, 16, 10) X(1, 6, 18)
#endif
#ifndef PTNN_PACK_FIXED
#define PTNN_PACK_FIXED(X) X(0, 4, 1, 5) X(0, 5, 1, 5)
#endif
#ifndef PTNN_PACKM_FIXED                // the same for the packed kernel over several CUs (segment_packm_kernel): Mackey-Glass 4-10-1
#define PTNN_PACKM_FIXED(X) X(0, 4, 1, 10)
#endif

namespace ptnn {
typedef void (*seg_fn)(const SegParams, const PersistParams, int);
typedef void (*model_fn)(const SegParams, int, const float*, const float*, float*, int, int);

// segment_pack_kernel<task, I, O, H> / segment_packm_kernel<task, I, O, H>: a packed kernel of a shape with the hidden width H
// compiled in (one per entry of PTNN_PACK_FIXED / PTNN_PACKM_FIXED, defined by ptnn_shape.hip with -DPTNN_HC (-DPTNN_HC_MULTI);
// ptnn.hip keeps the two lists and looks a handle's shape and width up in them)
struct PackFixed { int task, I, O, H; seg_fn pack; };

struct Shape {
    int task, I, O;
    seg_fn seg;             // cooperative schedule, H <= 64
    seg_fn spec;            // speculative schedule over work-groups, H <= 64
    model_fn model;
    seg_fn seg_wide;        // 64 < H <= 512
    model_fn model_wide;
    seg_fn pack;            // H <= 8: packed speculative schedule
    seg_fn tree;            // prefetching tree schedule (random-walk classification), H <= 64
    seg_fn seg_wide_res;    // 64 < H <= 512, H % 32 == 0, state + proposal resident in LDS
    int loops;              // which kernels carry the interval loop of a persistent launch: bit 0 seg, bit 1 pack (wide: always; spec, tree: never)
    int split_ch, split_kr; // split-operand forward pass (SplitK<I>): 16-byte chunks per image row (0: not available for this n_in), fp32 k-steps
    seg_fn packm;           // 9 <= H <= 16: packed schedule over several CUs per replica
};
}  // namespace ptnn
