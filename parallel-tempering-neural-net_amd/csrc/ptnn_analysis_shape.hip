// ptnn_analysis_shape.hip -- one (task, n_in, n_out) instantiation of every per-shape analysis kernel: compiled once per shape of
// ptnn_shapes.hpp with -DPTNN_T=<task> -DPTNN_I=<n_in> -DPTNN_O=<n_out> -DPTNN_SHAPE_SYMBOL=ptnn_ashape_<T>_<I>_<O>.
#include "ptnn_analysis_device.hpp"

using namespace ptnn;

extern "C" const AnalysisShape PTNN_SHAPE_SYMBOL = {PTNN_T, PTNN_I, PTNN_O,
                                                    &predict_forward_kernel<PTNN_T, PTNN_I, PTNN_O>, &forecast_forward_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                                    &sensitivity_forward_kernel<PTNN_T, PTNN_I, PTNN_O>, &pd_forward_kernel<PTNN_T, PTNN_I, PTNN_O>,
                                                    &shapley_forward_kernel<PTNN_T, PTNN_I, PTNN_O>, &ale_forward_kernel<PTNN_T, PTNN_I, PTNN_O>};
