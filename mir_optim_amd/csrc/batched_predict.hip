// batched_predict.hip -- the fitted curve and its confidence band of the batched path in FLOAT: the k_batched_predict instances
// (batched_predict.h) of ModelExpDecay, ModelExp3Affine and ModelExpDecayPad8 and their extern "C" entry. The double twin, with
// the 16-wide models, is batched_predict_d.hip; the entry itself is batched_predict_host.h.
#include "batched_predict_host.h"

using namespace mirlsq;

extern "C" int mir_lsq_batched_predict_s(const mir_least_squares_settings_s* S, size_t count, size_t q, int model, const float* x,
                                         const float* lower, const float* upper, const float* tq, size_t tq_stride,
                                         const float* covariance, float* value, float* sigma, const mir_lsq_batched_options* options,
                                         const mir_lsq_batched_extras* extras)
{
    return batched_predict_entry<float>([](int id, auto&& f) { return with_builtin_model<float>(id, f); }, S, count, q, model, x, lower, upper,
                                        tq, tq_stride, covariance, value, sigma, options, extras);
}
