// ptnn_shape.hip -- one (task, n_in, n_out) instantiation of every templated kernel: compiled once per shape of
// ptnn_shapes.hpp with -DPTNN_T=<task> -DPTNN_I=<n_in> -DPTNN_O=<n_out> -DPTNN_SHAPE_SYMBOL=ptnn_shape_<T>_<I>_<O>.
#include "ptnn_shapes.hpp"

#if !defined(PTNN_T) || !defined(PTNN_I) || !defined(PTNN_O) || !defined(PTNN_SHAPE_SYMBOL)
#error "compile with -DPTNN_T -DPTNN_I -DPTNN_O -DPTNN_SHAPE_SYMBOL"
#endif

using namespace ptnn;

#ifdef PTNN_SHAP
// ... or, with -DPTNN_SHAP on top (and its own PTNN_SHAPE_SYMBOL, ptnn_shap_<T>_<I>_<O>), nothing but the shape's coalition-value
// kernel (ptnn_dev_shapley.hpp): a code object of its own, so that the shape's other kernels keep their bytes
extern "C" const ShapShape PTNN_SHAPE_SYMBOL = {PTNN_T, PTNN_I, PTNN_O, &shapley_forward_kernel<PTNN_T, PTNN_I, PTNN_O>};
#elif defined(PTNN_HC)
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
                                            &segment_packm_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &predict_forward_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &forecast_forward_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &sensitivity_forward_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                            &pd_forward_kernel<PTNN_T, PTNN_I, PTNN_O>};
#endif
