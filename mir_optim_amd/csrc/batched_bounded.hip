// batched_bounded.hip -- the BOUNDED instances of the batched one-wavefront-per-problem fit in FLOAT: k_lm_batched<Model,
// WEIGHTED, BatchedBoxQpStep> (batched_bounded.h: the box QP of a bounded step solved inside the kernel) for ModelExpDecay, ModelExp3Affine and ModelExpDecayPad8,
// weighted and unweighted, behind MIR_LSQ_BATCHED_DEVICE_BOUNDS. A translation unit of its own: batched.hip, which holds the
// default instances and the extern "C" entries, compiles the device code it always compiled and reaches these six kernels
// through batched_bounded_enqueue (batched_host.h). No extern "C" symbol here.
#include "batched_host.h"

namespace mirlsq {

bool batched_bounded_enqueue(int model, const BatchedArgs<float>& a, bool weighted, size_t lds, hipStream_t stream)
{
    return batched_bounded_enqueue_builtin<float>(model, a, weighted, lds, stream);
}

}  // namespace mirlsq
