// fit_spline_gpu.hip -- fitSpline on DEVICE-RESIDENT points: mir_fit_spline_gpu_d / _s and mir_spline_eval_gpu_d / _s.
//
// fit_spline.cpp runs fitSpline (fit_splie.d:26-85) through the host-callback contract: every residual evaluation is a
// single-threaded pass over all points. Here the same residual function is the caller side of the GPU-native contract: f, fb and
// (double) fbRowMajorDiff with MIR_LSQ_FD_BASE_POINT are the kernels of fit_spline_kernels.h, enqueued on the solve's stream.
// The callbacks never synchronise and never allocate: every buffer (per-row interval and u, the coefficient table for
// p_max = 2 nx + 1 vectors, pen, the factor) is allocated once by the entry and freed after the solve has returned.
#include "driver.h"
#include "fit_spline_gpu.h"
#include "fit_spline_kernels.h"

using namespace mirlsq;

namespace spline_gpu {
namespace {

constexpr size_t kLdsLimit = 64 * 1024;

template <typename T>
struct Fit {
    hipStream_t stream = nullptr;
    size_t np = 0, nx = 0, m = 0, pmax = 0, nseg = 0;
    T lambda = 0;
    const T* points = nullptr;   // DEVICE np x 2 (nullptr: values only, no penalty row: the evaluation entry)
    void* block = nullptr;       // the one allocation the pointers below are carved from
    T *x = nullptr, *h = nullptr, *F = nullptr, *u = nullptr, *C = nullptr, *pen = nullptr, *dwork = nullptr, *Xup = nullptr;
    int32_t* seg = nullptr;
    int staged = 1;
    size_t lds = 0;
    bool failed = false;

    bool ok(hipError_t e) { if (e != hipSuccess) failed = true; return e == hipSuccess; }

    // rows: the abscissae are tp[i * stride], i < count; xup: room for an uploaded X of that many vectors (unit entries)
    int setup(size_t count, const T* tp, size_t stride, const T* xh, size_t xup)
    {
        nseg = nx > 1 ? nx - 1 : 1;
        const size_t lds_bytes = (4 + spline_c2::kFactorArrays) * nx * sizeof(T);
        staged = lds_bytes <= kLdsLimit;
        lds = staged ? lds_bytes : 0;
        std::vector<T> hh(nseg, T(0)), Fh(spline_c2::kFactorArrays * nx), work(nx);
        for (size_t i = 0; i + 1 < nx; ++i) hh[i] = xh[i + 1] - xh[i];
        spline_c2::c2_factor(nx, xh, Fh.data(), work.data());
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
        const size_t ox = take(nx * sizeof(T)), oh = take(nseg * sizeof(T)), oF = take(Fh.size() * sizeof(T));
        const size_t ou = take(count * sizeof(T)), os = take(count * sizeof(int32_t));
        const size_t oC = take(nseg * pmax * 4 * sizeof(T)), op = take(pmax * sizeof(T));
        const size_t od = take(staged ? 0 : pmax * nx * sizeof(T)), oX = take(xup * nx * sizeof(T));
        if (hipMalloc(&block, off ? off : 256) != hipSuccess) { block = nullptr; return -3; }
        char* b = static_cast<char*>(block);
        x = (T*)(b + ox); h = (T*)(b + oh); F = (T*)(b + oF); u = (T*)(b + ou); seg = (int32_t*)(b + os);
        C = (T*)(b + oC); pen = (T*)(b + op); dwork = (T*)(b + od); Xup = (T*)(b + oX);
        if (!ok(hipMemcpy(x, xh, nx * sizeof(T), hipMemcpyHostToDevice)) || !ok(hipMemcpy(h, hh.data(), nseg * sizeof(T), hipMemcpyHostToDevice))
            || !ok(hipMemcpy(F, Fh.data(), Fh.size() * sizeof(T), hipMemcpyHostToDevice)))
            return -5;
        if (count) {
            hipLaunchKernelGGL(k_spline_rows<T>, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, count, tp,
                               stride, nx, (const T*)x, seg, u);
            if (!ok(hipGetLastError())) return -5;
        }
        return 0;
    }
    void release()
    {
        if (block) (void)hipFree(block);
        block = nullptr;
    }

    void tables(size_t p, const T* X)
    {
        hipLaunchKernelGGL(k_spline_tables<T>, dim3((unsigned)p), dim3(kWaveLanes), lds, stream, nx, p, X, (const T*)x, (const T*)h,
                           (const T*)F, lambda, np, C, pen, dwork, staged);
        ok(hipGetLastError());
    }
    void point_rows(size_t rows, size_t p, T* Y)
    {
        hipLaunchKernelGGL(k_spline_points<T>, dim3((unsigned)((rows + kBlock - 1) / kBlock), (unsigned)p), dim3(kBlock), 0, stream,
                           rows, p, (const int32_t*)seg, (const T*)u, (const T*)h, (const T*)C, points ? (const T*)pen : (const T*)nullptr,
                           points, Y);
        ok(hipGetLastError());
    }
    // fb (f is p = 1): Y p x m point-major; more vectors than the table holds go in pieces
    void fb(size_t p, const T* X, T* Y)
    {
        for (size_t k0 = 0; k0 < p; k0 += pmax) {
            const size_t pc = p - k0 < pmax ? p - k0 : pmax;
            tables(pc, X + k0 * nx);
            point_rows(m, pc, Y + k0 * m);
        }
    }
    // fbRowMajorDiff: p = 2 nx or 2 nx + 1
    void fbd(size_t p, const T* X, T* D)
    {
        if (p != 2 * nx && p != 2 * nx + 1) { failed = true; return; }
        tables(p, X);
        int W = 1;
        while (W < kWaveLanes && (size_t)W < nx) W *= 2;
        const size_t rows_per_block = (size_t)(kBlock / W) * kDiffSteps;
        hipLaunchKernelGGL(k_spline_diff<T>, dim3((unsigned)((m + rows_per_block - 1) / rows_per_block)), dim3(kBlock), 0, stream, m, nx,
                           p, W, (const int32_t*)seg, (const T*)u, (const T*)h, (const T*)C, (const T*)pen, points, D);
        ok(hipGetLastError());
    }
};

template <typename T> void cb_f(void* c, size_t, size_t, const T* x, T* y) { static_cast<Fit<T>*>(c)->fb(1, x, y); }
template <typename T> void cb_fb(void* c, size_t, size_t, size_t p, const T* X, T* Y) { static_cast<Fit<T>*>(c)->fb(p, X, Y); }
template <typename T> void cb_fbd(void* c, size_t, size_t, size_t p, const T* X, T* D) { static_cast<Fit<T>*>(c)->fbd(p, X, D); }

template <typename T> struct Entry;
template <> struct Entry<double> {
    using S = mir_least_squares_settings_d; using R = mir_least_squares_result_d;
    static void init(S* s) { mir_least_squares_init_d(s); }
    static R run(const S* s, size_t m, size_t n, double* x, const double* l, const double* u, const mir_lsq_gpu_options* o, void* ctx)
    {
        return mir_optimize_least_squares_gpu_d(s, m, n, x, l, u, o, ctx, &cb_f<double>, nullptr, nullptr, nullptr, nullptr);
    }
    static void* diff() { return reinterpret_cast<void*>(&cb_fbd<double>); }
    static void derivatives(size_t n, const double* x, const double* y, double* d) { mir_spline_c2_derivatives_d(n, x, y, d); }
};
template <> struct Entry<float> {
    using S = mir_least_squares_settings_s; using R = mir_least_squares_result_s;
    static void init(S* s) { mir_least_squares_init_s(s); }
    static R run(const S* s, size_t m, size_t n, float* x, const float* l, const float* u, const mir_lsq_gpu_options* o, void* ctx)
    {
        return mir_optimize_least_squares_gpu_s(s, m, n, x, l, u, o, ctx, &cb_f<float>, nullptr, nullptr, nullptr, nullptr);
    }
    static void* diff() { return nullptr; }       // fbRowMajorDiff is f64-only in the solver
    static void derivatives(size_t n, const float* x, const float* y, float* d) { mir_spline_c2_derivatives_s(n, x, y, d); }
};

// the caller's options struct is versioned by struct_size: a member is read only when the struct covers it
#define SPLINE_COVERS(o, member) ((o)->struct_size >= offsetof(mir_lsq_gpu_options, member) + sizeof((o)->member))

template <typename T>
int fit_spline_gpu(const typename Entry<T>::S* settings, size_t np, const T* points, size_t nx, const T* x, const T* l, const T* u,
                   T lambda, const mir_lsq_gpu_options* opt, T* splineY, T* splineD, typename Entry<T>::R* result)
{
    // every argument check comes before the first HIP call: a machine without a GPU still gets the argument codes
    if (!points || !x || !l || !u || !splineY || !result || nx == 0 || np == 0 || !(lambda >= 0)) return MIR_FIT_SPLINE_BAD_ARGUMENT;
    if (opt) {
        if (opt->comm || opt->fb || opt->fbContext) return MIR_FIT_SPLINE_BAD_ARGUMENT;
        if (SPLINE_COVERS(opt, fbRowMajor) && opt->fbRowMajor) return MIR_FIT_SPLINE_BAD_ARGUMENT;
        if (SPLINE_COVERS(opt, fbRowMajorDiff) && opt->fbRowMajorDiff) return MIR_FIT_SPLINE_BAD_ARGUMENT;
    }
    if (np < nx && lambda == 0) return MIR_FIT_SPLINE_TOO_FEW_POINTS;              // FS:47-51
    typename Entry<T>::S defaults;
    if (!settings) { Entry<T>::init(&defaults); settings = &defaults; }
    for (size_t i = 0; i < nx; ++i) splineY[i] = 0;                                // FS:56-57
    typename Entry<T>::R none{};
    none.status = mir_ls_numericError;
    *result = none;
    if (!device_available()) return MIR_FIT_SPLINE_OK;                             // as mir_fit_spline_*: the status says it

    Fit<T> c;
    c.np = np; c.nx = nx; c.lambda = lambda; c.points = points;
    c.m = np + (lambda == 0 ? 1 : 0);                                              // FS:85
    c.pmax = 2 * nx + 1;
    c.stream = opt ? static_cast<hipStream_t>(opt->stream) : nullptr;
    const bool own_stream = c.stream == nullptr;
    if (own_stream && hipStreamCreate(&c.stream) != hipSuccess) return MIR_FIT_SPLINE_OK;
    if (c.setup(np, points, 2, x, 0) == 0) {
        mir_lsq_gpu_options o{};
        o.struct_size = sizeof(o);
        o.flags = MIR_LSQ_DEVICE_CALLBACKS | MIR_LSQ_FD_BASE_POINT;
        o.stream = c.stream;
        o.fbContext = &c;
        o.fb = reinterpret_cast<void*>(&cb_fb<T>);
        o.fbRowMajorDiff = Entry<T>::diff();
        if (opt) {
            o.flags |= opt->flags & MIR_LSQ_TIME_KERNELS;
            o.workspace = opt->workspace;
            o.variant = opt->variant;
            o.stats = opt->stats;
            if (SPLINE_COVERS(opt, trace)) o.trace = opt->trace;
            // the statistics keep the caller's version of the struct (header: "Versioning of mir_lsq_stats")
            size_t bytes = SPLINE_COVERS(opt, fbRowMajorDiff) ? offsetof(mir_lsq_stats, trial_callback_points) + sizeof(uint64_t)
                         : SPLINE_COVERS(opt, fbRowMajor)     ? offsetof(mir_lsq_stats, jtj_fd_launches) + sizeof(uint64_t)
                                                                                 : offsetof(mir_lsq_stats, qp_active_set_passes) + sizeof(uint64_t);
            if (SPLINE_COVERS(opt, stats_size) && opt->stats_size) bytes = opt->stats_size;
            o.stats_size = (uint32_t)(bytes < sizeof(mir_lsq_stats) ? bytes : sizeof(mir_lsq_stats));
        }
        *result = Entry<T>::run(settings, c.m, nx, splineY, l, u, &o, &c);
        (void)hipStreamSynchronize(c.stream);
        if (c.failed) result->status = mir_ls_numericError;                        // a callback's launch failed
    }
    c.release();
    if (own_stream) (void)hipStreamDestroy(c.stream);
    if (splineD) Entry<T>::derivatives(nx, x, splineY, splineD);
    return MIR_FIT_SPLINE_OK;
}

// values of the Hermite spline (x, y, d: HOST) at t[count] (DEVICE) -> out[count] (DEVICE): the table of ONE vector is built
// on the host with the statements of the fit, the rows go through k_spline_rows / k_spline_points
template <typename T>
int spline_eval_gpu(size_t n, const T* x, const T* y, const T* d, size_t count, const T* t, T* out, void* stream)
{
    if (n == 0 || !x || !y || !d || (count && (!t || !out))) return -1;
    if (count == 0) return 0;
    if (!device_available()) return -2;
    Fit<T> c;
    c.nx = n; c.pmax = 1; c.stream = static_cast<hipStream_t>(stream);
    int rc = c.setup(count, t, 1, x, 0);
    if (rc == 0) {
        std::vector<T> hh(c.nseg, T(0)), Ch(c.nseg * 4);
        for (size_t i = 0; i + 1 < n; ++i) hh[i] = x[i + 1] - x[i];
        for (size_t s = 0; s < c.nseg; ++s) spline_c2::segment_coeffs(n, hh.data(), y, d, s, Ch.data() + 4 * s);
        if (!c.ok(hipMemcpy(c.C, Ch.data(), Ch.size() * sizeof(T), hipMemcpyHostToDevice))) rc = -5;
    }
    if (rc == 0) {
        c.point_rows(count, 1, out);
        if (!c.ok(hipStreamSynchronize(c.stream)) || c.failed) rc = -5;          // the per-row scratch is freed below
    }
    c.release();
    return rc;
}

}  // namespace

template <typename T>
int callback_eval(size_t np, const T* points, size_t nx, const T* x, T lambda, size_t p, const T* Xh, int mode, T* out)
{
    if (!points || !x || !Xh || !out || nx == 0 || np == 0 || p == 0 || !(lambda >= 0) || (mode != 0 && mode != 1)) return -1;
    if (mode == 1 && (sizeof(T) != 8 || (p != 2 * nx && p != 2 * nx + 1))) return -1;
    if (!device_available()) return -2;
    Fit<T> c;
    c.np = np; c.nx = nx; c.lambda = lambda; c.points = points;
    c.m = np + (lambda == 0 ? 1 : 0);
    c.pmax = 2 * nx + 1;
    if (hipStreamCreate(&c.stream) != hipSuccess) return -5;
    const size_t nout = mode == 0 ? p * c.m : c.m * nx + (p == 2 * nx + 1 ? c.m : 0);
    T* Y = nullptr;
    int rc = c.setup(np, points, 2, x, p);
    if (rc == 0 && hipMalloc((void**)&Y, nout * sizeof(T)) != hipSuccess) rc = -3;
    if (rc == 0 && !c.ok(hipMemcpyAsync(c.Xup, Xh, p * nx * sizeof(T), hipMemcpyHostToDevice, c.stream))) rc = -5;
    if (rc == 0) {
        if (mode == 0) cb_fb<T>(&c, c.m, nx, p, c.Xup, Y);
        else cb_fbd<T>(&c, c.m, nx, p, c.Xup, Y);
        if (!c.ok(hipMemcpyAsync(out, Y, nout * sizeof(T), hipMemcpyDeviceToHost, c.stream)) || !c.ok(hipStreamSynchronize(c.stream)) || c.failed)
            rc = -5;
    }
    if (Y) (void)hipFree(Y);
    c.release();
    (void)hipStreamDestroy(c.stream);
    return rc;
}

template <typename T>
int host_eval(size_t np, const T* points, size_t nx, const T* x, T lambda, size_t p, const T* Xh, int mode, T* out)
{
    if (!points || !x || !Xh || !out || nx == 0 || np == 0 || p == 0 || !(lambda >= 0) || (mode != 0 && mode != 1)) return -1;
    if (mode == 1 && p != 2 * nx && p != 2 * nx + 1) return -1;
    const size_t m = np + (lambda == 0 ? 1 : 0), nseg = nx > 1 ? nx - 1 : 1;
    std::vector<T> h(nseg, T(0)), F(spline_c2::kFactorArrays * nx), d(nx), u(np), C(nseg * p * 4), pen(p);
    std::vector<int32_t> seg(np);
    for (size_t i = 0; i + 1 < nx; ++i) h[i] = x[i + 1] - x[i];
    spline_c2::c2_factor(nx, x, F.data(), d.data());
    host_rows(np, points, 2, nx, x, seg.data(), u.data());
    for (size_t k = 0; k < p; ++k)
        vector_tables(nx, x, h.data(), F.data(), Xh + k * nx, d.data(), lambda, np, p, k, C.data(), pen.data());
    if (mode == 0) host_points(m, p, seg.data(), u.data(), h.data(), C.data(), pen.data(), points, out);
    else host_diff(m, nx, p, seg.data(), u.data(), h.data(), C.data(), pen.data(), points, out);
    return 0;
}

template <typename T>
int factor(size_t nx, const T* x, T* F)
{
    if (nx == 0 || !x || !F) return -1;
    std::vector<T> work(nx);
    spline_c2::c2_factor(nx, x, F, work.data());
    return 0;
}

template int callback_eval<double>(size_t, const double*, size_t, const double*, double, size_t, const double*, int, double*);
template int callback_eval<float>(size_t, const float*, size_t, const float*, float, size_t, const float*, int, float*);
template int host_eval<double>(size_t, const double*, size_t, const double*, double, size_t, const double*, int, double*);
template int host_eval<float>(size_t, const float*, size_t, const float*, float, size_t, const float*, int, float*);
template int factor<double>(size_t, const double*, double*);
template int factor<float>(size_t, const float*, float*);

}  // namespace spline_gpu

extern "C" {

int mir_fit_spline_gpu_d(const mir_least_squares_settings_d* settings, size_t npoints, const double* points, size_t nx,
                         const double* x, const double* l, const double* u, double lambda, const mir_lsq_gpu_options* options,
                         double* splineY, double* splineD, mir_least_squares_result_d* result)
{
    return spline_gpu::fit_spline_gpu<double>(settings, npoints, points, nx, x, l, u, lambda, options, splineY, splineD, result);
}
int mir_fit_spline_gpu_s(const mir_least_squares_settings_s* settings, size_t npoints, const float* points, size_t nx,
                         const float* x, const float* l, const float* u, float lambda, const mir_lsq_gpu_options* options,
                         float* splineY, float* splineD, mir_least_squares_result_s* result)
{
    return spline_gpu::fit_spline_gpu<float>(settings, npoints, points, nx, x, l, u, lambda, options, splineY, splineD, result);
}
int mir_spline_eval_gpu_d(size_t n, const double* x, const double* y, const double* d, size_t count, const double* t, double* out,
                          void* stream)
{
    return spline_gpu::spline_eval_gpu<double>(n, x, y, d, count, t, out, stream);
}
int mir_spline_eval_gpu_s(size_t n, const float* x, const float* y, const float* d, size_t count, const float* t, float* out,
                          void* stream)
{
    return spline_gpu::spline_eval_gpu<float>(n, x, y, d, count, t, out, stream);
}

}  // extern "C"
