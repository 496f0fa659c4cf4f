// batched_predict_host.h -- the extern "C" entries of the fitted curve and its confidence band (mir_lsq_batched_predict_s / _d,
// mir_lsq_batched16_predict_d) for the compiled-in models: launch_batched_predict<Model> of include/mir_optim_amd_batched.hpp
// behind the dispatch from the model id (with_builtin_model / with_builtin_model16, batched_host.h). The argument checks are the
// launch's own (detail::predict_arguments) plus the plausibility of the options, all answered -1 before a device is looked for
// (-2), the order every batched entry keeps. batched_predict.hip (float) and batched_predict_d.hip (double: n <= 8 and the 16-wide
// models) instantiate k_batched_predict -- units of their own, so that every other unit compiles what it always compiled.
#pragma once

#include "batched_host.h"

namespace mirlsq {

// Dispatch: f(Model{}) by the model id, -1 for an id of the other family (BuiltinModels<T> or BuiltinModels16<...>::with_model)
template <class T, class Dispatch>
int batched_predict_entry(Dispatch&& with_model, const typename Abi<T>::Settings* S, size_t count, size_t q, int model, const T* x,
                          const T* lower, const T* upper, const T* tq, size_t tq_stride, const T* covariance, T* value, T* sigma,
                          const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return with_model(model, [&](auto mdl) {
        using Model = decltype(mdl);
        if (!batched_options_plausible(options)) return -1;
        const mir_lsq_batched_options o = batched_options(options);
        mir_lsq_batched_extras e;
        if (!mir_optim_amd::detail::predict_arguments<Model>(S, count, q, x, lower, upper, tq, tq_stride, covariance, value, sigma, &o, extras, e))
            return -1;
        if (count == 0 || q == 0) return 0;
        if (!device_available()) return -2;
        return mir_optim_amd::launch_batched_predict<Model>(S, count, q, x, lower, upper, tq, tq_stride, covariance, value, sigma, &o, extras);
    });
}

}  // namespace mirlsq
