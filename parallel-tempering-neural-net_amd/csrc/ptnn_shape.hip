// ptnn_shape.hip -- one (task, n_in, n_out) instantiation of every templated kernel of the sampler: compiled once per shape of
// ptnn_shapes.hpp with -DPTNN_T=<task> -DPTNN_I=<n_in> -DPTNN_O=<n_out> -DPTNN_SHAPE_SYMBOL=ptnn_shape_<T>_<I>_<O> (analysis: ptnn_analysis_shape.hip).
#include "ptnn_shapes.hpp"

#if !defined(PTNN_T) || !defined(PTNN_I) || !defined(PTNN_O) || !defined(PTNN_SHAPE_SYMBOL)
#error "compile with -DPTNN_T -DPTNN_I -DPTNN_O -DPTNN_SHAPE_SYMBOL"
#endif

using namespace ptnn;

#ifdef PTNN_HC
// ... or, with -DPTNN_HC=<n_hidden> on top (and its own PTNN_SHAPE_SYMBOL, ptnn_pack_fixed_<T>_<I>_<O>_<H>), nothing but the shape's
// packed kernel with that hidden width compiled in
// (-DPTNN_HC_MULTI, ptnn_packm_fixed_<T>_<I>_<O>_<H>: the kernel over several CUs)
#ifdef PTNN_HC_MULTI
extern "C" const PackFixed PTNN_SHAPE_SYMBOL = {PTNN_T, PTNN_I, PTNN_O, PTNN_HC, &segment_packm_kernel<PTNN_T, PTNN_I, PTNN_O, PTNN_HC>};
#else
extern "C" const PackFixed PTNN_SHAPE_SYMBOL = {PTNN_T, PTNN_I, PTNN_O, PTNN_HC, &segment_pack_kernel<PTNN_T, PTNN_I, PTNN_O, PTNN_HC>};
#endif
#else
extern "C" const Shape PTNN_SHAPE_SYMBOL = {PTNN_T, PTNN_I, PTNN_O,
                                            &segment_kernel<PTNN_T, PTNN_I, PTNN_O>, &segment_spec_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &model_kernel<PTNN_T, PTNN_I, PTNN_O>, &segment_wide_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &model_wide_kernel<PTNN_T, PTNN_I, PTNN_O>, &segment_pack_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &segment_tree_kernel<PTNN_T, PTNN_I, PTNN_O>, &segment_wide_res_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            (coop_has_loop<PTNN_T, PTNN_I, PTNN_O>() ? 1 : 0) | (pack_has_loop<PTNN_T, PTNN_I, PTNN_O>() ? 2 : 0),
                                            SplitK<PTNN_I>::OK ? SplitK<PTNN_I>::CH : 0, SplitK<PTNN_I>::KR,
                                            &segment_packm_kernel<PTNN_T, PTNN_I, PTNN_O>};
#endif
