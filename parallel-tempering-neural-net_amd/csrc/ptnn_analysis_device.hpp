// ptnn_analysis_device.hpp -- the per-shape device code of the posterior analysis calls, and its per-shape kernel table.
// The rule: `Shape` (ptnn_shapes.hpp) holds the sampler's kernels; `AnalysisShape` holds every per-shape analysis kernel; a new
// one is added there.  The sampler's code objects are held to their bytes (compare_device_code.py) and a kernel added to a code
// object moves the addresses and the LDS kernel ids of its other kernels, so a shape's analysis kernels have a code object of their
// own, ptnn_ashape_<T>_<I>_<O> (ptnn_analysis_shape.hip), and ptnn.hip, ptnn_shape.hip and ptnn_checkpoint.hip see none of this.
// ptnn_analysis.hip launches the kernels through the table.  ptnn_device.hpp provides WAVE, the math, the work-group helpers and
// `#pragma clang fp contract(off)`, which governs the parts below (textually included, inside namespace ptnn) as it does the sampler.
#pragma once
#include "ptnn_device.hpp"

namespace ptnn {
#include "ptnn_dev_net.hpp"                  // the network itself, stated once: arguments, staging, row load, decode, sigmoids, output head
#include "ptnn_dev_predict.hpp"              // posterior predictive: the forward pass (selection and reduction: ptnn_dev_select.hpp)
#include "ptnn_dev_forecast.hpp"             // recursive multi-step forecasts: the recursive forward pass
#include "ptnn_dev_sensitivity.hpp"          // input sensitivity: the forward pass that carries the derivative to the inputs
#include "ptnn_dev_pd.hpp"                   // partial dependence and ICE curves: the forward pass over substituted inputs
#include "ptnn_dev_shapley.hpp"              // coalition values (Shapley attributions): the forward pass over hybrid rows
#include "ptnn_dev_ale.hpp"                  // accumulated local effects: the forward pass over each row's own bin edges

struct AnalysisShape {
    int task, I, O;
    void (*predict_fwd)(const PredictFwd);   // posterior predictive: network outputs of distinct vectors x input rows (every H)
    void (*forecast_fwd)(const ForecastFwd); // recursive forecasts: trajectories x origins x horizon steps (REG, n_out == 1; else empty)
    void (*sens_fwd)(const SensFwd);         // input sensitivity: d output / d input of distinct vectors x input rows (every H)
    void (*pd_fwd)(const PdFwd);             // partial dependence: outputs of distinct vectors x input rows x substituted grid values (every H)
    void (*shap_fwd)(const ShapFwd);         // coalition values: linear functionals of the game, distinct vectors x explained rows (every H)
    void (*ale_fwd)(const AleFwd);           // accumulated local effects: first and second differences across each row's own bin (every H)
};
}  // namespace ptnn
