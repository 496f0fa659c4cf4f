// batched_predict_d.hip -- the fitted curve and its confidence band of the batched path in DOUBLE: the k_batched_predict
// instances (batched_predict.h) of ModelExpDecayD, ModelExp3AffineD, ModelExpDecayPad8D (MIR_LSQ_MODEL_*) and of the two models of
// 9 to 16 parameters (MIR_LSQ_MODEL16_*), and their extern "C" entries: each answers -1 to the other family's ids. The float twin
// is batched_predict.hip; the entry itself is batched_predict_host.h.
#include "batched_predict_host.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_predict_d(const mir_least_squares_settings_d* S, size_t count, size_t q, int model, const double* x,
                              const double* lower, const double* upper, const double* tq, size_t tq_stride, const double* covariance,
                              double* value, double* sigma, const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return batched_predict_entry<double>([](int id, auto&& f) { return with_builtin_model<double>(id, f); }, S, count, q, model, x, lower,
                                         upper, tq, tq_stride, covariance, value, sigma, options, extras);
}

int mir_lsq_batched16_predict_d(const mir_least_squares_settings_d* S, size_t count, size_t q, int model, const double* x,
                                const double* lower, const double* upper, const double* tq, size_t tq_stride, const double* covariance,
                                double* value, double* sigma, const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return batched_predict_entry<double>([](int id, auto&& f) { return with_builtin_model16(id, f); }, S, count, q, model, x, lower, upper, tq,
                                         tq_stride, covariance, value, sigma, options, extras);
}

}  // extern "C"
