// batched_kernel.h -- many small independent LM fits, ONE WAVEFRONT PER PROBLEM (BASELINE cfg 5:
// 4096 x (m = 512, n = 8), fp32). The whole loop of optimizeLeastSquaresImplGeneric!T
// (/root/reference/source/mir/optim/least_squares.d:877-1176) runs inside the kernel:
//   * a wave (= a workgroup) owns one problem; its J (m x n), y and the trial residual live in LDS, lane l owns rows
//     l, l + 64, ...; x, dx and all scalars are replicated in registers, J^T J and J^T y are held one row per lane;
//   * the residual model is a compile-time functor (no callback across the FFI in this entry);
//   * finite-difference Jacobian (LS:1018-1049), Broyden (LS:1002-1006), J^T J / J^T y as per-lane partial sums
//     + one wave reduction, the n x n damped solve with one matrix row per lane (?posvx semantics: equilibrate,
//     Cholesky, refine: posvx_rows), acceptance and the lambda/mu schedule exactly as the reference;
//   * all control flow is wave-uniform, there is no barrier and no host round trip.
// A problem whose step hits a finite bound: the default instances do not finish it (BOXCQP's active-set loop is not part of
// them): it returns status kBatchedNeedsGeneral and the host entry re-solves it with the general solver. The BOUNDED instances
// (third template parameter of k_lm_batched, batched_bounded.h; MIR_LSQ_BATCHED_DEVICE_BOUNDS) solve the step's box QP in
// place, as the reference does (LS:1074-1085), and never return that status.
#pragma once

#include "common.h"
#include "solve_types.h"

namespace mirlsq {

constexpr int kBatchedNeedsGeneral = -100;
constexpr int kBatchedNMax = 8;

enum : int { kModelExpDecay = 0, kModelExp3Affine = 1, kModelExpDecayPad8 = 2 };

// ---- residual models: r_i = Model::eval(t_i, basis_i, x) - data_i. The contract of a model (the built-in ones below and
// any user model handed to launch_batched<Model>, include/mir_optim_amd_batched.hpp) -- the compile-time counterpart of the
// reference's residual callback f(x, y) (least_squares.d:73-80), restricted to residuals that are a function of ONE abscissa:
//     using value_type = double;   optional: the precision T of the whole fit, float (the default, when the member is absent)
//                                  or double (LeastSquaresSettings!double, the reference's main instantiation)
//     static constexpr int n;      number of parameters, 1 <= n <= 8
//     static constexpr int nb;     per-row BASIS values that do not depend on the parameters (0 = none)
//     __device__ static void basis(T t, T* b);                       fills b[0 .. nb)
//     __device__ static T eval(T t, const T* b, const T* x);         the model value at t; x has 8 entries, x[n..] = 0
// The basis values of every row are tabulated once per launch (k_batched_basis: rows x nb values of T) and eval() reads the
// row's values instead of evaluating them again at every trial point and finite-difference point: the same numbers enter the
// same expression. eval must be pure (the reference declares its callbacks pure) and wave-uniform in control flow.
template <class Model, class = void> struct batched_value { using type = float; };
template <class Model> struct batched_value<Model, std::void_t<typename Model::value_type>> { using type = typename Model::value_type; };
template <class Model> using batched_value_t = typename batched_value<Model>::type;

// the operations the kernel spells out, one overload per value type. A fused multiply-add is __builtin_elementwise_fma: ONE
// rounding (llvm.fma) in float or double, contraction being off in the kernel. It is a builtin, not a wrapper function, on
// purpose: a call of an inline overload reorders the IR enough that the fp32 kernels scheduled differently (the same operations
// in another order); with the builtin their code is the one __builtin_fmaf gave, instruction for instruction. The others are
// the IEEE operations of the type (the float ones are the calls the fp32 kernel always made).
__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float vmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float vabs(float a) { return fabsf(a); }
__device__ __forceinline__ double vabs(double a) { return fabs(a); }
__device__ __forceinline__ float vsqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ double vsqrt(double a) { return sqrt(a); }
// a decimal constant in T: the float literal for float (exactly the value the fp32 kernel always used), the double one else
template <class T> __host__ __device__ constexpr T lit(float f, double d) { return std::is_same<T, float>::value ? T(f) : T(d); }
struct ModelExpDecay {          // p0 exp(-t p1) + p2            (n = 3; reference unittest T5's family)
    static constexpr int n = 3, nb = 0;
    __device__ static inline void basis(float, float*) {}
    __device__ static inline float eval(float t, const float*, const float* x) { return x[0] * __expf(-t * x[1]) + x[2]; }
};
struct ModelExp3Affine {        // sum_{k<3} p_{2k} exp(-t p_{2k+1}) + p6 + p7 t   (n = 8)
    static constexpr int n = 8, nb = 0;
    __device__ static inline void basis(float, float*) {}
    __device__ static inline float eval(float t, const float*, const float* x)
    {
        return x[0] * __expf(-t * x[1]) + x[2] * __expf(-t * x[3]) + x[4] * __expf(-t * x[5]) + x[6] + x[7] * t;
    }
};
// exp(y) in float, the SAME bits on the device and on a host: every operation is written out (Cody-Waite reduction with a
// two-part ln 2, degree-7 Taylor polynomial on |r| <= ln 2 / 2: truncation 5e-9, ldexp) and is exactly rounded on both sides
// (fmaf, rintf, ldexpf); ~1.5 ulp. The float oracle's fused variant (oracle/lm_batched_fused.c) repeats it instruction for
// instruction, which libm's / the device library's expf would not allow (both are "<= 1 ulp", not the same ulp).
__host__ __device__ inline float det_expf(float y)
{
#pragma clang fp contract(off)
    // the ends behave as expf's do (round-4 advice: a clamp made exp(NaN) finite, so the reference's numericError exit on a
    // non-finite trial residual, LS:1117-1122, could not fire through this term): NaN stays NaN, overflow is +inf above
    // ln(FLT_MAX), and below -87 -- where the result would leave the normal range, which device and host ldexpf need not treat
    // alike -- the value is 0 (the true one is < 1.7e-38)
    if (!(y == y)) return y;
    if (y > 88.7228394f) return __builtin_huge_valf();
    if (y < -87.0f) return 0.0f;
    const float k = rintf(y * 1.44269504f);
    float r = __builtin_fmaf(k, -0.693145752f, y);
    r = __builtin_fmaf(k, -1.42860677e-06f, r);
    float p = 1.0f / 5040.0f;
    p = __builtin_fmaf(p, r, 1.0f / 720.0f);
    p = __builtin_fmaf(p, r, 1.0f / 120.0f);
    p = __builtin_fmaf(p, r, 1.0f / 24.0f);
    p = __builtin_fmaf(p, r, 1.0f / 6.0f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return ldexpf(p, (int)k);
}

// BASELINE cfg 5's well-conditioned n = 8 family ("p0 exp(-t p1) + p2 + 5-term variants padded to n = 8"): the
// exponential decay plus five terms that are LINEAR in their parameters (a two-frequency trigonometric pair and a slope),
// so the only nonlinearity is the decay and J^T J stays well conditioned in fp32. The four trigonometric values of a row are
// its basis (tabulated once a launch: device sinf / cosf; the fused oracle takes the table as an input). eval is ONE chain of
// fused multiply-adds around det_expf, nothing left to the compiler: the fused float oracle reproduces a fit of this model
// bit for bit (tests/test_gpu_batched.py); the libm oracle evaluates the same expression with expf and agrees to fp32 rounding.
struct ModelExpDecayPad8 {
    static constexpr int n = 8, nb = 4;
    __device__ static inline void basis(float t, float* b)
    {
        b[0] = sinf(2.0f * t); b[1] = cosf(2.0f * t); b[2] = sinf(5.0f * t); b[3] = cosf(5.0f * t);
    }
    __device__ static inline float eval(float t, const float* b, const float* x)
    {
#pragma clang fp contract(off)
        const float e = det_expf(-t * x[1]);
        float v = __builtin_fmaf(x[0], e, x[2]);
        v = __builtin_fmaf(x[3], b[0], v);
        v = __builtin_fmaf(x[4], b[1], v);
        v = __builtin_fmaf(x[5], b[2], v);
        v = __builtin_fmaf(x[6], b[3], v);
        return __builtin_fmaf(x[7], t, v);
    }
};
// ---- the same three models in DOUBLE (mir_optimize_least_squares_batched_d: same ids, same formulas). Device exp / sin / cos
// of the type; no host twin reproduces their bits, and none is needed: the f64 path is compared with the f64 oracle to tolerance.
struct ModelExpDecayD {
    using value_type = double;
    static constexpr int n = 3, nb = 0;
    __device__ static inline void basis(double, double*) {}
    __device__ static inline double eval(double t, const double*, const double* x) { return x[0] * exp(-t * x[1]) + x[2]; }
};
struct ModelExp3AffineD {
    using value_type = double;
    static constexpr int n = 8, nb = 0;
    __device__ static inline void basis(double, double*) {}
    __device__ static inline double eval(double t, const double*, const double* x)
    {
        return x[0] * exp(-t * x[1]) + x[2] * exp(-t * x[3]) + x[4] * exp(-t * x[5]) + x[6] + x[7] * t;
    }
};
struct ModelExpDecayPad8D {     // the basis table holds doubles
    using value_type = double;
    static constexpr int n = 8, nb = 4;
    __device__ static inline void basis(double t, double* b)
    {
        b[0] = sin(2.0 * t); b[1] = cos(2.0 * t); b[2] = sin(5.0 * t); b[3] = cos(5.0 * t);
    }
    __device__ static inline double eval(double t, const double* b, const double* x)
    {
        return x[0] * exp(-t * x[1]) + x[2] + x[3] * b[0] + x[4] * b[1] + x[5] * b[2] + x[6] * b[3] + x[7] * t;
    }
};
// the compiled-in models of mir_optimize_least_squares_batched_s / _d by their MIR_LSQ_MODEL_* id and value type
template <int ID, class T> struct BuiltinModel;
template <> struct BuiltinModel<kModelExpDecay, float> { using type = ModelExpDecay; };
template <> struct BuiltinModel<kModelExp3Affine, float> { using type = ModelExp3Affine; };
template <> struct BuiltinModel<kModelExpDecayPad8, float> { using type = ModelExpDecayPad8; };
template <> struct BuiltinModel<kModelExpDecay, double> { using type = ModelExpDecayD; };
template <> struct BuiltinModel<kModelExp3Affine, double> { using type = ModelExp3AffineD; };
template <> struct BuiltinModel<kModelExpDecayPad8, double> { using type = ModelExpDecayPad8D; };

// T = float: the layout of mir_least_squares_result_s (24 bytes); T = double: of mir_least_squares_result_d (32 bytes)
template <class T> struct BatchedResult { int32_t status; uint32_t iterations, fCalls, gCalls; T residual, lambda; };

template <class T> struct BatchedArgs {
    LmSettingsDev<T> set;
    uint32_t maxIterations, maxAge;
    int count, m;
    const T* t;            // m (shared) or count x m
    int t_stride;          // 0 = shared
    const T* data;         // count x m
    T* x;                  // count x n, in/out
    const T* lower;        // n (shared: b_stride 0) or count x n (b_stride n: row k is problem k's box)
    const T* upper;        // as lower
    BatchedResult<T>* results;
    const T* basis;        // (t_stride ? count : 1) x m x nb: the model's per-row basis (k_batched_basis), nullptr when nb == 0
    uint64_t* timing;      // profiling builds (MIRLSQ_BATCHED_TIMING): 10 x count cycle counters (mir_lsq_batched_options.timing), else unused
    uint32_t variant;      // kBatchedNoLadder: one damping value per solve (A/B and the test of the ladder against it)
    int w_stride;          // 0 = one vector of m weights shared by all problems, m = count x m
    const T* weights;      // the WEIGHTED instances only (k_lm_batched<Model, true>): the residual of row i is w_i (eval - data_i)
    int b_stride;          // 0 = one box of n values for all problems, n = count x n (MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM): read by
                           // k_lm_batched16; for k_lm_batched the host picks the OWN_BOX instance from it
};
constexpr uint32_t kBatchedNoLadder = 1u;
constexpr uint32_t kBatchedAnalytic = 2u;      // MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN: Model::grad instead of finite differences

// a model MAY provide the derivative of its value with respect to the parameters -- the reference's optional g callback
// (least_squares.d:80, 1010-1014):   __device__ static void grad(T t, const T* b, const T* x, T* gi /* n */);
template <class Model, class = void> struct batched_has_grad : std::false_type {};
template <class Model>
struct batched_has_grad<Model, std::void_t<decltype(Model::grad(batched_value_t<Model>(0), (const batched_value_t<Model>*)nullptr,
                                                                (const batched_value_t<Model>*)nullptr,
                                                                (batched_value_t<Model>*)nullptr))>> : std::true_type {};

// one row of the basis table: 16-byte loads when the model has four values
template <int NB, class T = float> struct BasisRow {
    T v[NB > 0 ? NB : 1];
    __device__ inline void load(const T* table, int i)
    {
        if constexpr (NB == 4 && std::is_same<T, float>::value) {
            const float4 q = reinterpret_cast<const float4*>(table)[i];
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else if constexpr (NB == 4) {
            const double2 q0 = reinterpret_cast<const double2*>(table)[2 * i], q1 = reinterpret_cast<const double2*>(table)[2 * i + 1];
            v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
        } else {
#pragma unroll
            for (int k = 0; k < NB; ++k) v[k] = table[(size_t)i * NB + k];
        }
    }
};

template <class Model>
__global__ __launch_bounds__(256) void k_batched_basis(const batched_value_t<Model>* __restrict__ t,
                                                       batched_value_t<Model>* __restrict__ table, size_t rows)
{
    constexpr int NB = Model::nb;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < rows; i += (size_t)gridDim.x * blockDim.x) {
        batched_value_t<Model> b[NB > 0 ? NB : 1];
        Model::basis(t[i], b);
#pragma unroll
        for (int k = 0; k < NB; ++k) table[i * NB + k] = b[k];
    }
}

// ---- the damped n x n solve with ONE ROW PER LANE ------------------------------------------------------------------------
// ?posvx('E','L') as the oracle restates it (oracle/lm_oracle_impl.inc, lmo_posvx: ?poequ, ?laqsy, ?potf2, ?potrs, ?porfs;
// the condition estimate is left out: the reference accepts info = n + 1, boxcqp.d:212, and reads no other output of it).
// Lane r = lane & 7 of every group of eight lanes holds row r of each matrix (eight registers a matrix instead of the 36 of a
// private copy per lane, which took 256 + 29 registers and ~2000 instructions a solve) and component r of each vector; the
// eight groups of a wave compute the same thing. A value of another row comes through v_readlane (lanes 0..7 hold every row).
// Every element sees the operations of the oracle's loops in the oracle's order: the left-looking sums of ?potf2
// (`s -= F[i][k] F[j][k]`, k ascending) are applied one k at a time to the whole trailing part; the forward sweep of ?potrs
// runs by columns, its backward sweep (a chain that can only start when z[i + 1] is known) in lane i on column i of the
// factor. Every multiply-add is ONE fused operation (__builtin_elementwise_fma), division and square root are the IEEE ones: the result
// equals, bit for bit, the oracle's float ?posvx written with fmaf in the same loops (oracle/lm_oracle.c, lmo_posvx_fused_s;
// tests/test_gpu_batched.py) -- and this file does not depend on which products the compiler chooses to fuse.
// Divisions and square roots per solve: 44 + 9 sequences (a copy per lane: 76 + 16). The same template serves double.
__device__ inline float lane_get(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ inline double lane_get(double v, int k)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}
// a[r], r = lane & 7, as a chain of selects on VALUES: taking the array by reference lets the optimiser turn the chain into one
// load at a computed address, which pins the whole array in scratch memory
template <class T> __device__ inline T row_pick8(T a0, T a1, T a2, T a3, T a4, T a5, T a6, T a7, int r)
{
    T v = a0;
    v = (r == 1) ? a1 : v; v = (r == 2) ? a2 : v; v = (r == 3) ? a3 : v; v = (r == 4) ? a4 : v;
    v = (r == 5) ? a5 : v; v = (r == 6) ? a6 : v; v = (r == 7) ? a7 : v;
    return v;
}
#define MIRLSQ_ROW_PICK(a, r) row_pick8((a)[0], (a)[1], (a)[2], (a)[3], (a)[4], (a)[5], (a)[6], (a)[7], (r))
// max / min over the eight rows (every lane gets it): the values repeat with period 8 along a 16-lane DPP row, so the
// rotations by 4, 2, 1 pair each lane with the rows r ^ 4, then r ^ 2, r ^ 1. fmax / fmin: a NaN operand is ignored.
template <class T> __device__ inline T rows_max(T v)
{
    v = vmax(v, dpp_row_ror<4>(v)); v = vmax(v, dpp_row_ror<2>(v)); v = vmax(v, dpp_row_ror<1>(v));
    return v;
}
template <class T> __device__ inline T rows_min(T v)
{
    v = vmin(v, dpp_row_ror<4>(v)); v = vmin(v, dpp_row_ror<2>(v)); v = vmin(v, dpp_row_ror<1>(v));
    return v;
}

// ?posvx('E','L'), n = N <= NMAX = 8, FOUR SYSTEMS A WAVE: each row of 16 lanes (a DPP row; r = lane & 7, the upper eight lanes
// repeat the lower eight) solves its own system, so that one call serves a ladder of four damping values (k_lm_batched).
// Prow: the full symmetric row r of this group's P; rhs_r: component r of its right-hand side. x: the group's solution in every
// lane of the group. Returns the group's info in every lane of the group. There is no branch on a group's data: a group whose
// factorization fails keeps computing on values nobody reads.
// MASKED (boxqp_rows.h: the reduced systems of the active-set loop, solved in place at full order as posvx_rows16 does): only
// the rows with live_r belong to the group's system, `order` of them; the row and column of every other index are the
// identity's and its right-hand side is 0, which leaves the arithmetic of the live part exactly that of the compact system in
// the reference's order (every skipped term is an exact zero), and ?poequ, berr and safe1 look at the live rows only. The
// unmasked instantiations ignore both arguments and are, operation for operation, what they were before the parameter existed.
template <int N, int NMAX, class T, bool MASKED = false>
__device__ inline int posvx_rows(const T (&Prow)[NMAX], T rhs_r, int r, T (&x)[NMAX], bool live_r = true, int order = N)
{
    static_assert(NMAX == 8, "row r = lane & 7");
    const T eps = Lim<T>::eps / 2, safmin = Lim<T>::min_normal;
    const bool live = MASKED ? (r < N && live_r) : r < N;
    const T d_r = MIRLSQ_ROW_PICK(Prow, r);
    // ?poequ
    const T smin = rows_min(live ? d_r : Lim<T>::inf());
    const T amax = rows_max(live ? d_r : -Lim<T>::inf());
    const bool pos = smin > 0;
    const T scond = vsqrt(smin) / vsqrt(amax);
    const T s_r = (pos && live) ? T(1) / vsqrt(d_r) : T(1);
    const T small = safmin / Lim<T>::eps, large = T(1) / small;
    const bool rcequ = pos && !(scond >= lit<T>(0.1f, 0.1) && amax >= small && amax <= large);
    // ?laqsy
    T Arow[NMAX], Frow[NMAX], Fcol[NMAX], s[NMAX];               // Fcol[k] = F[k][r], k > r: column r of the factor, for L^T
    static_for<NMAX>([&](auto K) {
        constexpr int k = K.value;
        s[k] = dpp_row_bcast<k>(s_r);
        const T v = Prow[k];
        bool lk = true;                                              // column k belongs to the system
        if constexpr (MASKED) lk = dpp_row_bcast<k>(live ? 1 : 0) != 0;
        Arow[k] = (live && k < N && lk) ? (rcequ ? s[k] * s_r * v : v) : (r == k ? T(1) : T(0));
        Frow[k] = Arow[k];
        Fcol[k] = T(0);
    });
    const T b_r = live ? (rcequ ? s_r * rhs_r : rhs_r) : T(0);
    // ?potf2 'L': after step j, Frow[jj] (jj > j) of row r >= jj holds A[r][jj] - sum_{k <= j} F[r][k] F[jj][k]
    int info = 0;
    static_for<NMAX>([&](auto J) {
        constexpr int j = J.value;
        if constexpr (j < N) {
            T ajj = dpp_row_bcast<j>(Frow[j]);
            info = (info == 0 && !(ajj > 0)) ? j + 1 : info;
            ajj = vsqrt(ajj);
            const T q = Frow[j] / ajj;
            Frow[j] = (r == j) ? ajj : q;                          // rows above the diagonal carry values nobody reads
            static_for<NMAX>([&](auto JJ) {
                constexpr int jj = JJ.value;
                if constexpr (jj > j && jj < N) {
                    const T ljj = dpp_row_bcast<jj>(Frow[j]);      // F[jj][j]
                    Frow[jj] = __builtin_elementwise_fma(-Frow[j], ljj, Frow[jj]);
                    Fcol[jj] = (r == j) ? ljj : Fcol[jj];
                }
            });
        }
    });
    const T fd_r = MIRLSQ_ROW_PICK(Frow, r);                      // F[r][r]
    // ?potrs. L y = v by columns: row r takes `t -= F[r][i] y[i]` at step i (ascending i, as in the oracle's row loop).
    // L^T z = y: row i needs t = y[i] - sum_{k > i} F[k][i] z[k] with k ascending, a chain that can only start when z[i + 1]
    // is known: lane i runs it on its column of the factor and the group's z[k].
    auto potrs = [&](T v_r, T (&z)[NMAX]) {
        static_for<NMAX>([&](auto I) {
            constexpr int i = I.value;
            if constexpr (i < N) {
                const T yi = dpp_row_bcast<i>(v_r / fd_r);
                const T upd = __builtin_elementwise_fma(-Frow[i], yi, v_r);
                v_r = (r == i) ? yi : (r > i ? upd : v_r);
            }
        });
#pragma unroll
        for (int i = 0; i < NMAX; ++i) z[i] = T(0);
        static_for<NMAX>([&](auto II) {
            constexpr int i = NMAX - 1 - II.value;
            if constexpr (i < N) {
                T t = v_r;
#pragma unroll
                for (int k = 0; k < NMAX; ++k) if (k > i && k < N) t = __builtin_elementwise_fma(-Fcol[k], z[k], t);
                z[i] = dpp_row_bcast<i>(t / fd_r);
            }
        });
    };
    potrs(b_r, x);
    // ?porfs: the loop runs while any group refines; a group that has stopped keeps its solution
    const T safe1 = (T)((MASKED ? order : N) + 1) * safmin, safe2 = safe1 / eps;
    T lstres = 3;
    bool active = true;
    for (int count = 1;; ++count) {
        T ri = b_r, wi = vabs(b_r);
#pragma unroll
        for (int k = 0; k < NMAX; ++k) if (k < N) {
            ri = __builtin_elementwise_fma(-Arow[k], x[k], ri);
            wi = __builtin_elementwise_fma(vabs(Arow[k]), vabs(x[k]), wi);
        }
        const bool big = wi > safe2;
        const T q = (big ? vabs(ri) : vabs(ri) + safe1) / (big ? wi : wi + safe1);
        const T berr = rows_max(live ? q : T(0));
        active = active && berr > eps && 2 * berr <= lstres && count <= 5;
        if (__builtin_amdgcn_ballot_w64(active) == 0) break;
        T c[NMAX];
        potrs(live ? ri : T(0), c);
#pragma unroll
        for (int i = 0; i < NMAX; ++i) x[i] = active ? x[i] + c[i] : x[i];
        lstres = active ? berr : lstres;
    }
#pragma unroll
    for (int i = 0; i < NMAX; ++i) x[i] = rcequ ? s[i] * x[i] : x[i];
    return info;
}

// unit-test entry of posvx_rows: four systems a wave; P count x 64 (row-major, lower triangle read), rhs and x count x 8
template <int N, class T = float>
__global__ __launch_bounds__(64) void k_posvx_rows(const T* __restrict__ P, const T* __restrict__ rhs, int count,
                                                   T* __restrict__ x, int* __restrict__ info)
{
    const int lane = threadIdx.x, r = lane & 7, g = lane >> 4;
    for (int p0 = 4 * blockIdx.x; p0 < count; p0 += 4 * gridDim.x) {
        const int p = p0 + g < count ? p0 + g : count - 1;            // a short last wave repeats the last system
        T Prow[8], sol[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) Prow[k] = (r < N && k < N) ? P[(size_t)p * 64 + (k <= r ? r * 8 + k : k * 8 + r)] : T(0);
        const int rc = posvx_rows<N, 8>(Prow, r < N ? rhs[(size_t)p * 8 + r] : T(0), r, sol);
        if ((lane & 15) == 0 && p0 + g < count) {
            info[p] = rc;
#pragma unroll
            for (int k = 0; k < 8; ++k) x[(size_t)p * 8 + k] = (rc == 0 && k < N) ? sol[k] : T(0);
        }
    }
}

// -DMIRLSQ_BATCHED_TIMING: per problem, the shader-clock cycles (s_memtime) spent in [0] residual evaluations, [1] Jacobian
// refreshes (FD or Broyden), [2] J^T J / J^T y with its reductions, [3] damped solves, [4] the whole fit, and [5] the number of
// solve calls, [6] a trial's preparation, [7] an accepted step's bookkeeping, [8] the box QPs of a bounded instance, written to BatchedArgs::timing (10 x uint64 a problem). A profiling build only (scripts/probes/cfg5_phases.py).
#ifdef MIRLSQ_BATCHED_TIMING
#define MIRLSQ_T0() const uint64_t t0_ = __builtin_readcyclecounter()
#define MIRLSQ_T1(k) tacc[k] += __builtin_readcyclecounter() - t0_
#else
#define MIRLSQ_T0() ((void)0)
#define MIRLSQ_T1(k) ((void)0)
#endif

// waves per SIMD: float, what the LDS slices allow at m = 512; double, one -- which lets the compiler use the whole file of
// 512 VGPRs + AGPRs (the f64 ladder, J^T J accumulators and vectors need about twice the fp32 kernel's registers: DESIGN
// section 9). LDS bounds the f64 occupancy near there anyway: a problem at m = 512, n = 8 takes 40 KiB of a CU's 160.
template <class Model> constexpr int batched_waves_per_simd()
{
    return std::is_same<batched_value_t<Model>, double>::value ? 1 : (Model::n <= 4 ? 4 : 2);
}

// WEIGHTED (a compile-time parameter: the host picks the instance, launch_batched): the residual of row i is
// w_i (eval(t_i, b_i, x) - data_i) -- ONE multiplication after the subtraction, wherever a residual or a Jacobian row is formed
// (feval; the finite-difference points, each weighted before they are differenced, which is what the reference sees through a
// weighted f; J_ij = w_i g_j on the analytic path). The weights are read from global memory next to t and data, in the same
// chunked, clamped loads: no LDS, the m limits stay. A weight of exactly 0 removes its row (residual and Jacobian row are zero):
// a batch of problems of different lengths is padded to a common m with zero-weight rows. Non-finite weights are the caller's
// error: a NaN residual takes the reference's numericError exits. The unweighted instances do not read a.weights and are,
// instruction for instruction, what they were before the parameter existed.
// Bounds: what the kernel does with a damped step that leaves the box. BatchedNoBoundedStep (the default): the problem returns
// kBatchedNeedsGeneral, as it always did. BatchedBoxQpStep (batched_bounded.h, which includes boxqp_rows.h; this header knows
// neither): Bounds::step<N>(...) replaces the step by the solution of the box QP of LS:1074-1085. The default instances do
// not see the parameter: they are, instruction for instruction, what they were before it existed.
struct BatchedNoBoundedStep { static constexpr bool enabled = false; };
constexpr uint32_t kBatchedDeviceBounds = 4u;  // MIR_LSQ_BATCHED_DEVICE_BOUNDS: the host launches a bounded instance (the kernel does not read the bit)

// OWN_BOX (MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM; the host picks the instance from BatchedArgs::b_stride, as it picks WEIGHTED):
// lower / upper hold count x n values and the problem takes row `prob`, wave-uniform address arithmetic once at entry. A
// compile-time parameter and not the run-time stride the other kernels read, because the shared-bounds launch of two families
// (EXP_DECAY_PAD8 f32 default, f64 bounded) measured outside the spread of two runs of the parent with it
// (profiles/r18/batched_problem_bounds.txt): the shared-bounds instances do not read b_stride and are, instruction for
// instruction, what they were before per-problem bounds existed.
template <class Model, bool WEIGHTED = false, class Bounds = BatchedNoBoundedStep, bool OWN_BOX = false>
__global__ __launch_bounds__(64, batched_waves_per_simd<Model>()) void k_lm_batched(BatchedArgs<batched_value_t<Model>> a)
{
    // Nothing in this body is left to the compiler's choice of what to fuse: contraction is off and every multiply-add that is
    // meant to be ONE rounding is a __builtin_elementwise_fma. The arithmetic of a fit is then a fixed sequence of IEEE operations that
    // oracle/lm_batched_fused.c repeats on the host for float (per-lane partial sums, the butterfly of wave_sum): bit-identical
    // results. T = double runs the same sequence in double.
#pragma clang fp contract(off)
    using T = batched_value_t<Model>;
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "Model::value_type: float or double");
    constexpr int N = Model::n;
    constexpr int NMAX = kBatchedNMax;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    // one problem per (single-wave) workgroup: the dispatcher hands a finished wave's slot to the next problem, so a
    // long fit delays nobody (four problems per workgroup held three slots until the slowest of the four was done)
    const int lane = threadIdx.x;
    const int prob = blockIdx.x;
    const int m = a.m;
    T* Jl = reinterpret_cast<T*>(smem_b);                                  // J: m x N row-major
    T* yv = Jl + (size_t)N * m;
    T* mB = yv + m;
    const T* tp = a.t + (size_t)(a.t_stride ? prob : 0) * a.t_stride;
    const T* dp = a.data + (size_t)prob * m;
    constexpr int NB = Model::nb;
    const T* bp = NB ? a.basis + (size_t)(a.t_stride ? prob : 0) * a.t_stride * NB : nullptr;
    const LmSettingsDev<T>& S = a.set;
    const T* wp = nullptr;
    if constexpr (WEIGHTED) wp = a.weights + (size_t)(a.w_stride ? prob : 0) * a.w_stride;
    const T* lop = a.lower;
    const T* upp = a.upper;
    if constexpr (OWN_BOX) {                              // the problem's own row
        lop += (size_t)prob * N;
        upp += (size_t)prob * N;
    }

    T x[NMAX], lo[NMAX], up[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        x[j] = j < N ? a.x[(size_t)prob * N + j] : T(0);
        lo[j] = j < N ? lop[j] : -Lim<T>::inf();
        up[j] = j < N ? upp[j] : Lim<T>::inf();
    }
#ifdef MIRLSQ_BATCHED_TIMING
    uint64_t tacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t tstart = __builtin_readcyclecounter();
#endif
    BatchedResult<T> ret;
    ret.status = -26;   // numericError, LS:132
    ret.iterations = 0; ret.fCalls = 0; ret.gCalls = 0;
    ret.residual = Lim<T>::inf(); ret.lambda = 0;

    // The lane's rows (lane, lane + 64, ...) are taken in chunks of UNR: the loads of a chunk are issued together (index clamped
    // to the last row: always a valid address), then the rows are used in order, so a wave does not pay one memory latency a
    // row. The sum of squares is accumulated in the order of the plain loop.
    auto feval = [&](const T (&p)[NMAX], T* dst) -> T {                  // dst = f(p); returns ||f||^2
        constexpr int UNR = 8;
        T ss = 0;
        for (int base = lane; base - lane < m; base += kWave * UNR) {
            T tv[UNR], dv[UNR], rv[UNR], wv[WEIGHTED ? UNR : 1];
            BasisRow<NB, T> bv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = min(base + kWave * u, m - 1);
                tv[u] = tp[i]; dv[u] = dp[i];
                if constexpr (WEIGHTED) wv[u] = wp[i];
                bv[u].load(bp, i);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                rv[u] = Model::eval(tv[u], bv[u].v, p) - dv[u];
                if constexpr (WEIGHTED) rv[u] = wv[u] * rv[u];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = base + kWave * u;
                if (i < m) dst[i] = rv[u];
                ss = i < m ? __builtin_elementwise_fma(rv[u], rv[u], ss) : ss;
            }
        }
        return wave_sum(ss);
    };

    // validation LS:930-943 (settings were checked on the host; x / bounds here)
    bool finite = true, inb = true;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) if (j < N) {
        if (!(-Lim<T>::inf() < x[j] && x[j] < Lim<T>::inf())) finite = false;
        if (!(lo[j] <= x[j]) || !(x[j] <= up[j])) inb = false;
    }
    if (m == 0 || !finite) ret.status = -31;           // badGuess
    else if (!inb) ret.status = -32;                   // badBounds
    else {
        constexpr bool HAS_GRAD = batched_has_grad<Model>::value;
        const bool use_g = HAS_GRAD && (a.variant & kBatchedAnalytic) != 0;  // g of LS:1010-1014 (the launcher refuses it without grad)
        const uint32_t maxAge = a.maxAge ? a.maxAge : (use_g ? 3u : 2u * N);     // LS:945
        { MIRLSQ_T0(); ret.residual = feval(x, yv); MIRLSQ_T1(0); }       // LS:953-955
        ++ret.fCalls;
        bool fConverged = LM_F_CONVERGED(ret.residual, S);
        bool needJacobian = true;
        uint32_t age = maxAge;
        // J^T J and J^T y live one ROW per lane (row r = lane & 7 in every group of eight lanes), as posvx_rows wants them
        const int r = lane & 7;
        T dx[NMAX], JJrow[NMAX], Jy_r = 0;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) { dx[j] = 0; JJrow[j] = 0; }
        T lad_x[NMAX], lad_lam[4] = {0, 0, 0, 0};          // the ladder of solutions (group g of the wave: level g), see below
#pragma unroll
        for (int j = 0; j < NMAX; ++j) lad_x[j] = 0;
        int lad_info = 0, lad_level = 0;
        bool lad_valid = false;
        const int lad_depth = (a.variant & kBatchedNoLadder) ? 1 : 4;
        T dx_dot = 0, mu = 1, lambda = 0;
        ret.status = -1;                                                   // maxIterations, LS:971
        do {
            if (fConverged) { ret.status = 3; break; }                     // LS:974
            if (!LM_LAMBDA_IN_RANGE(lambda, S)) { ret.status = 0; break; } // LS:979
            if (mu > kSuspiciousMu && age) { needJacobian = true; age = maxAge; mu = 1; }   // LS:984
            {
                bool nan = false;
#pragma unroll
                for (int j = 0; j < NMAX; ++j) if (j < N && !(x[j] <= x[j])) nan = true;
                if (nan) { ret.status = -26; break; }                      // LS:990
            }
            if (needJacobian) {                                            // LS:996
                needJacobian = false;
                MIRLSQ_T0();
                if (age < maxAge) {                                        // Broyden LS:999-1007
                    age++;
                    const T d = T(1) / dx_dot;
                    for (int i = lane; i < m; i += kWave) {
                        T* Ji = Jl + (size_t)i * N;
                        T dot = 0;
#pragma unroll
                        for (int j = 0; j < N; ++j) dot = __builtin_elementwise_fma(Ji[j], dx[j], dot);
                        const T t = (mB[i] - yv[i]) + dot;                 // mB holds the previous residual
                        const T u = -d * t;
#pragma unroll
                        for (int j = 0; j < N; ++j) Ji[j] = __builtin_elementwise_fma(u, dx[j], Ji[j]);
                    }
                } else if (use_g) {                                        // g(x, J), LS:1010-1014
                    age = 0;
                    if constexpr (HAS_GRAD) {
                        for (int i = lane; i < m; i += kWave) {
                            BasisRow<NB, T> b;
                            b.load(bp, i);
                            T gi[NMAX];
#pragma unroll
                            for (int j = 0; j < NMAX; ++j) gi[j] = 0;
                            Model::grad(tp[i], b.v, x, gi);
                            if constexpr (WEIGHTED) {
                                const T wi = wp[i];
#pragma unroll
                                for (int j = 0; j < N; ++j) gi[j] = wi * gi[j];
                            }
#pragma unroll
                            for (int j = 0; j < N; ++j) Jl[(size_t)i * N + j] = gi[j];
                        }
                    }
                    ++ret.gCalls;                                          // LS:1013
                } else {                                                   // FD LS:1016-1050
                    age = 0;
                    // the n central differences of a row share its t, d and basis: rows outside, columns inside
                    T xph[NMAX], xmh[NMAX], inv[NMAX];
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) {
                        xmh[j] = vmax(x[j] - S.jacobianEpsilon, lo[j]);
                        xph[j] = vmin(x[j] + S.jacobianEpsilon, up[j]);
                        const T twh = xph[j] - xmh[j];
                        inv[j] = twh != 0 ? T(1) / twh : T(0);             // a zero-width interval: the column is zero, LS:1045
                    }
                    for (int i = lane; i < m; i += kWave) {
                        BasisRow<NB, T> b;
                        b.load(bp, i);
                        const T ti = tp[i], di = dp[i];
                        T wi = 1;
                        if constexpr (WEIGHTED) wi = wp[i];
                        T p[NMAX];
#pragma unroll
                        for (int k = 0; k < NMAX; ++k) p[k] = x[k];
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            p[j] = xph[j];
                            T fp = Model::eval(ti, b.v, p) - di;
                            if constexpr (WEIGHTED) fp = wi * fp;
                            p[j] = xmh[j];
                            T fm = Model::eval(ti, b.v, p) - di;
                            if constexpr (WEIGHTED) fm = wi * fm;
                            p[j] = x[j];
                            const T v = fp - fm;
                            Jl[(size_t)i * N + j] = inv[j] != 0 ? v * inv[j] : T(0);
                        }
                    }
                    ret.fCalls += N;                                       // LS:1049 (quirk Q5)
                }
#ifdef MIRLSQ_BATCHED_TIMING
                const uint64_t t1_ = __builtin_readcyclecounter();
                tacc[1] += t1_ - t0_;
#endif
                // Jy = J^T y (LS:1052) and JJ = J^T J lower (LS:1065) in one sweep over the lane's rows
                T accJ[NMAX][NMAX], accy[NMAX];
#pragma unroll
                for (int j = 0; j < NMAX; ++j) { accy[j] = 0;
#pragma unroll
                    for (int k = 0; k < NMAX; ++k) accJ[j][k] = 0; }
                for (int i = lane; i < m; i += kWave) {
                    const T* Ji = Jl + (size_t)i * N;
                    const T yi = yv[i];
                    T row[NMAX];
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) row[j] = j < N ? Ji[j] : T(0);
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        accy[j] = __builtin_elementwise_fma(row[j], yi, accy[j]);
#pragma unroll
                        for (int k = 0; k <= j; ++k) accJ[j][k] = __builtin_elementwise_fma(row[j], row[k], accJ[j][k]);
                    }
                }
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const T ty = wave_sum(accy[j]);
                    Jy_r = (r == j) ? ty : Jy_r;
#pragma unroll
                    for (int k = 0; k <= j; ++k) {
                        const T t = wave_sum(accJ[j][k]);                      // element (j, k) and its mirror (k, j)
                        JJrow[k] = (r == j) ? t : JJrow[k];
                        if (k != j) JJrow[j] = (r == k) ? t : JJrow[j];
                    }
                }
                lad_valid = false;                                             // J^T J has changed
#ifdef MIRLSQ_BATCHED_TIMING
                tacc[2] += __builtin_readcyclecounter() - t1_;
#endif
                const T gmax = lane_get(rows_max(vabs(Jy_r)), 0);              // rows >= N hold zeros
                if (!(gmax > S.gradTolerance)) {                           // LS:1053-1062
                    if (age == 0) { ret.status = 2; break; }
                    age = maxAge;
                    continue;
                }
            }
            if (!LM_LAMBDA_SET(lambda, S)) {                               // LS:1067-1072
                // the largest diagonal element (a sum of squares: its own absolute value; a NaN is skipped as by `>`)
                const T best = lane_get(rows_max(r < N ? vabs(MIRLSQ_ROW_PICK(JJrow, r)) : T(-1)), 0);
                LM_LAMBDA0(lambda, best < 0 ? T(0) : best, S);
            }
            // LS:1079-1080 (-> QP:194). The four 16-lane groups of the wave solve with lambda and with the three values the
            // rejection rule (LS:1101-1106, 1125-1130: lambda *= lambdaIncrease mu, mu *= 2) would make of it next, at the
            // cost of one solve; a rejected step then finds its solution ready. A level is used only while J^T J is the one
            // the ladder was built on and lambda is bit for bit the ladder's value: the steps are those of the one-by-one loop.
            if (!(lad_valid && lad_level < lad_depth && lambda == lad_lam[lad_level])) {
                T l = lambda, mm = mu;
#pragma unroll
                for (int g = 0; g < 4; ++g) { lad_lam[g] = l; LM_REJECT(l, mm, S); }
                const int g = lane >> 4;
                const T mine = g == 0 ? lad_lam[0] : (g == 1 ? lad_lam[1] : (g == 2 ? lad_lam[2] : lad_lam[3]));
                T Prow[NMAX];
#pragma unroll
                for (int k = 0; k < NMAX; ++k) Prow[k] = JJrow[k] + ((k == r && r < N) ? mine : T(0));   // (Q1)
                MIRLSQ_T0();
                lad_info = posvx_rows<N, NMAX>(Prow, -Jy_r, r, lad_x);
                MIRLSQ_T1(3);
#ifdef MIRLSQ_BATCHED_TIMING
                ++tacc[5];
#endif
                lad_level = 0;
                lad_valid = true;
            }
#ifdef MIRLSQ_BATCHED_TIMING
            const uint64_t t6_ = __builtin_readcyclecounter();
#endif
            T sol[NMAX];
            const int lad_lane = 16 * lad_level++;
            const int info = __builtin_amdgcn_readlane(lad_info, lad_lane);
#pragma unroll
            for (int j = 0; j < NMAX; ++j) sol[j] = lane_get(lad_x[j], lad_lane);
            if (info != 0) { ret.status = -26; break; }
            bool feasible = true, nan = false;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) if (j < N) {
                if (!((lo[j] - x[j]) <= sol[j] && sol[j] <= (up[j] - x[j]))) feasible = false;   // QP:216-219
                if (!(sol[j] <= sol[j])) nan = true;
            }
            if constexpr (Bounds::enabled) {
                // LS:1074-1085: the box QP of this level's system (P = J^T J + this level's lambda: the level is used only while
                // lambda is bit for bit the ladder's value), started from the level's unconstrained solution. The ladder is not
                // touched: its other levels stay valid across rejections.
                if (!feasible) {
                    MIRLSQ_T0();
                    const bool solved = Bounds::template step<N>(JJrow, Jy_r, lambda, lo, up, x, S, r, lane >> 4, sol);
                    MIRLSQ_T1(8);
                    if (!solved) { ret.status = -26; break; }              // LS:1083
                    nan = false;
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) if (j < N && !(sol[j] <= sol[j])) nan = true;
                }
                if (nan) { ret.status = -26; break; }                      // LS:1087
            } else {
                if (nan) { ret.status = -26; break; }                      // LS:1087
                if (!feasible) { ret.status = kBatchedNeedsGeneral; break; }   // active-set loop: general solver
            }
            T trial[NMAX], ndd = 0;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) {
                T d = sol[j] + x[j];                                       // LS:1096-1097
                d = d - x[j];
                sol[j] = j < N ? d : T(0);
                ndd = __builtin_elementwise_fma(sol[j], sol[j], ndd);
                trial[j] = vmax(vmin(sol[j] + x[j], up[j]), lo[j]);        // LS:1108-1110
            }
            if (!LM_STEP_ALLOWED(vsqrt(ndd), S)) { LM_REJECT(lambda, mu, S); continue; }   // LS:1101-1106
            ++ret.fCalls;                                                  // LS:1112-1115
#ifdef MIRLSQ_BATCHED_TIMING
            tacc[6] += __builtin_readcyclecounter() - t6_;
#endif
            // the trial residual goes to the buffer that is NOT the current y
            T trialResidual;
            { MIRLSQ_T0(); trialResidual = feval(trial, mB); MIRLSQ_T1(0); }
            if (!(trialResidual <= Lim<T>::inf())) { ret.status = -26; break; }       // LS:1117
            const T improvement = ret.residual - trialResidual;
#ifdef MIRLSQ_BATCHED_TIMING
            const uint64_t t7_ = __builtin_readcyclecounter();
#endif
            if (!(improvement > 0)) { LM_REJECT(lambda, mu, S); continue; }   // LS:1125-1130
            needJacobian = true;                                           // LS:1132-1139
            mu = 1;
            ret.iterations++;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) { x[j] = trial[j]; dx[j] = sol[j]; }
            { T* tmp = yv; yv = mB; mB = tmp; }                            // swap(mBuffer, y): mB = previous residual
            ret.residual = trialResidual;
            fConverged = LM_F_CONVERGED(ret.residual, S);
            dx_dot = ndd;
            T pred = 0;                                                    // LS:1141-1142 (undamped JJ)
            {
                T tj = 0;                                                  // row r of J^T J dx + 2 J^T y, then the dot with dx
#pragma unroll
                for (int k = 0; k < NMAX; ++k) tj = __builtin_elementwise_fma(JJrow[k], dx[k], tj);
                tj = tj + 2 * Jy_r;
#pragma unroll
                for (int j = 0; j < NMAX; ++j) pred = __builtin_elementwise_fma(lane_get(tj, j), dx[j], pred);
            }
            pred = -pred;
            if (!(pred > 0)) { ret.status = 0; break; }                    // LS:1144-1148
            const T rho = pred / improvement;                              // LS:1150 (Q2)
            LM_RATE_STEP(rho, lambda, mu, S);                              // LS:1152-1161
            T xn = 0;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) xn = __builtin_elementwise_fma(x[j], x[j], xn);
#ifdef MIRLSQ_BATCHED_TIMING
            tacc[7] += __builtin_readcyclecounter() - t7_;
#endif
            if (!LM_X_MOVING(vsqrt(dx_dot), vsqrt(xn), S)) {               // LS:1164-1173 (Q6)
                if (age == 0) { ret.status = 1; break; }
                age = maxAge;
                continue;
            }
        } while (ret.iterations < a.maxIterations);                        // LS:1175
        ret.lambda = lambda;
    }
#ifdef MIRLSQ_BATCHED_TIMING
    tacc[4] = __builtin_readcyclecounter() - tstart;
    if (lane == 0 && a.timing) for (int k = 0; k < 10; ++k) a.timing[(size_t)prob * 10 + k] = tacc[k];
#endif
    if (lane == 0) {
        a.results[prob] = ret;
#pragma unroll
        for (int j = 0; j < N; ++j) a.x[(size_t)prob * N + j] = x[j];
    }
}


// ---- covariance of the fitted parameters, one wave per problem, no LDS, on the stream of the fit after it ---------------------
//     cov = s^2 (J^T J)^-1,   s^2 = ||f(x)||^2 / (rows with a nonzero weight - n),   or s^2 = 1 with kBatchedAbsoluteSigma
// (the pcov of a curve fit; with weights w_i = 1 / sigma_i and kBatchedAbsoluteSigma it is the covariance in the units of sigma).
// J is rebuilt row by row at the final x exactly as a refresh of the fit kernel builds it (Model::grad with kBatchedAnalytic,
// else central differences with jacobianEpsilon clipped to the bounds; weighted rows), J^T J is accumulated as there (per-lane
// partial sums in the row order of the fit, then wave_sum) and inverted by posvx_rows on unit right-hand sides: the four 16-lane
// groups take four columns a call. ||f(x)||^2 and the status are read from the fit's result record. The n x n values of a
// problem are written row-major, symmetric (the mean of the two solves' mirror elements). Degenerate cases:
//     status < 0 (also -100 from the kernel entry: that problem is not finished)   every entry NaN
//     a non-positive minor in the factorization, or rows - n_free <= 0              every free entry +inf
// The box is the problem's own (b_stride n) or the shared one (0). A parameter with l_j == u_j in it is FIXED (the rule of the
// general solver's covariance, covariance.hip; one that merely sits on a bound with l_j < u_j is not): its Jacobian column is
// not formed (zeroed on the grad path), its index is taken out of the system (unit diagonal, zero off-diagonal), row j and
// column j of the result are exactly 0, and n above is n_free, the number of parameters that are not fixed. A problem without
// a fixed parameter computes, operation for operation, what it computed before the rule existed.
template <class T> struct BatchedCovArgs {
    T jacobianEpsilon;
    int count, m;
    const T* t; int t_stride;
    const T* data;
    const T* x;            // count x n: the fitted parameters
    const T* lower; const T* upper;
    const BatchedResult<T>* results;
    const T* basis;
    const T* weights; int w_stride;      // nullptr = unweighted
    uint32_t variant;      // kBatchedAnalytic
    uint32_t flags;        // kBatchedAbsoluteSigma
    T* cov;                // count x n x n
    int b_stride;          // 0 = lower / upper hold n values for all problems, n = count x n
};
constexpr uint32_t kBatchedAbsoluteSigma = 1u;      // MIR_LSQ_BATCHED_ABSOLUTE_SIGMA

template <class Model>
__global__ __launch_bounds__(64) void k_batched_covariance(BatchedCovArgs<batched_value_t<Model>> a)
{
#pragma clang fp contract(off)
    using T = batched_value_t<Model>;
    constexpr int N = Model::n, NMAX = kBatchedNMax, NB = Model::nb;
    const int lane = threadIdx.x, prob = blockIdx.x, m = a.m, r = lane & 7;
    T* out = a.cov + (size_t)prob * N * N;
    const int status = a.results[prob].status;
    if (status < 0) {
        if (lane < N * N) out[lane] = Lim<T>::inf() - Lim<T>::inf();       // NaN
        return;
    }
    const T* tp = a.t + (size_t)(a.t_stride ? prob : 0) * a.t_stride;
    const T* dp = a.data + (size_t)prob * m;
    const T* bp = NB ? a.basis + (size_t)(a.t_stride ? prob : 0) * a.t_stride * NB : nullptr;
    const T* wp = a.weights ? a.weights + (size_t)(a.w_stride ? prob : 0) * a.w_stride : nullptr;
    const T* lop = a.lower + (size_t)prob * a.b_stride;   // the problem's own box, or the shared one (b_stride 0)
    const T* upp = a.upper + (size_t)prob * a.b_stride;
    T x[NMAX], xph[NMAX], xmh[NMAX], inv[NMAX];
    unsigned fix = 0;                                     // bit j: l_j == u_j, parameter j is fixed (wave-uniform)
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        x[j] = j < N ? a.x[(size_t)prob * N + j] : T(0);
        const T lo = j < N ? lop[j] : -Lim<T>::inf(), up = j < N ? upp[j] : Lim<T>::inf();
        const bool fixed_j = j < N && lo == up;
        fix |= fixed_j ? 1u << j : 0u;
        xmh[j] = vmax(x[j] - a.jacobianEpsilon, lo);
        xph[j] = vmin(x[j] + a.jacobianEpsilon, up);
        const T twh = xph[j] - xmh[j];
        inv[j] = (twh != 0 && !fixed_j) ? T(1) / twh : T(0);        // 0: the column of a fixed parameter is not formed
    }
    const int nfree = N - __builtin_popcount(fix);
    constexpr bool HAS_GRAD = batched_has_grad<Model>::value;
    const bool use_g = HAS_GRAD && (a.variant & kBatchedAnalytic) != 0;
    T accJ[NMAX][NMAX], rows = 0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
#pragma unroll
        for (int k = 0; k < NMAX; ++k) accJ[j][k] = 0;
    for (int i = lane; i < m; i += kWave) {
        BasisRow<NB, T> b;
        b.load(bp, i);
        const T ti = tp[i], di = dp[i], wi = wp ? wp[i] : T(1);
        rows += wi != 0 ? T(1) : T(0);
        T row[NMAX];
#pragma unroll
        for (int j = 0; j < NMAX; ++j) row[j] = 0;
        if (use_g) {
            if constexpr (HAS_GRAD) {
                Model::grad(ti, b.v, x, row);
                if (wp) {
#pragma unroll
                    for (int j = 0; j < N; ++j) row[j] = wi * row[j];
                }
#pragma unroll
                for (int j = 0; j < N; ++j) row[j] = ((fix >> j) & 1u) ? T(0) : row[j];      // a fixed parameter has no column
            }
        } else {
            T p[NMAX];
#pragma unroll
            for (int k = 0; k < NMAX; ++k) p[k] = x[k];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                p[j] = xph[j];
                T fp = Model::eval(ti, b.v, p) - di;
                p[j] = xmh[j];
                T fm = Model::eval(ti, b.v, p) - di;
                p[j] = x[j];
                if (wp) { fp = wi * fp; fm = wi * fm; }
                const T v = fp - fm;
                row[j] = inv[j] != 0 ? v * inv[j] : T(0);
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j)
#pragma unroll
            for (int k = 0; k <= j; ++k) accJ[j][k] = __builtin_elementwise_fma(row[j], row[k], accJ[j][k]);
    }
    T JJrow[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) JJrow[j] = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            const T s = wave_sum(accJ[j][k]);
            JJrow[k] = (r == j) ? s : JJrow[k];
            if (k != j) JJrow[j] = (r == k) ? s : JJrow[j];
        }
    // the index of a fixed parameter is taken out of the system: unit diagonal, zero off-diagonal (posvx_rows then factors an
    // SPD matrix whose free part is the reduced problem's J^T J). Without a fixed parameter every select keeps its value.
    const bool fixed_r = ((fix >> r) & 1u) != 0;
#pragma unroll
    for (int k = 0; k < NMAX; ++k) JJrow[k] = (fixed_r || ((fix >> k) & 1u)) ? (r == k ? T(1) : T(0)) : JJrow[k];
    const T dof = wave_sum(rows) - T(nfree);             // row counts are small integers: exact in T
    // column c = 4 call + g of the inverse by group g = lane >> 4: the right-hand side is the unit vector e_c
    const int g = lane >> 4;
    T sol[2][NMAX];
    int info = posvx_rows<N, NMAX>(JJrow, (r == g && r < N) ? T(1) : T(0), r, sol[0]);
    if constexpr (N > 4) info |= posvx_rows<N, NMAX>(JJrow, (r == 4 + g && r < N) ? T(1) : T(0), r, sol[1]);
    info = __builtin_amdgcn_readlane(info, 0);            // the four groups factor the same matrix
    const T s2 = (a.flags & kBatchedAbsoluteSigma) ? T(1) : a.results[prob].residual / dof;
    const bool degenerate = info != 0 || !(dof > 0);
    T mine = 0;                                           // lane i n + c takes element (i, c)
    static_for<NMAX>([&](auto I) {
        constexpr int i = I.value;
        static_for<NMAX>([&](auto Cc) {
            constexpr int c = Cc.value;
            if constexpr (i < N && c < N) {
                const T vic = lane_get(sol[c / 4][i], 16 * (c & 3)), vci = lane_get(sol[i / 4][c], 16 * (i & 3));
                const T v = s2 * ((vic + vci) / 2);
                mine = (lane == i * N + c) ? v : mine;
            }
        });
    });
    // row and column of a fixed parameter: exactly 0, in the degenerate case too
    const int oi = lane / N, oc = lane - oi * N;
    const bool fixed_out = (((fix >> oi) | (fix >> oc)) & 1u) != 0;
    if (lane < N * N) out[lane] = fixed_out ? T(0) : (degenerate ? Lim<T>::inf() : mine);
}

// residual of one problem as a DEVICE callback body (used when a batched problem falls back to the general solver); w: the
// problem's m weights, or nullptr
template <class Model, class T = batched_value_t<Model>>
__global__ __launch_bounds__(256) void k_batched_model_eval(const T* __restrict__ t, const T* __restrict__ d,
                                                            const T* __restrict__ x, T* __restrict__ y, int m,
                                                            const T* __restrict__ w)
{
    constexpr int NB = Model::nb;
    T p[kBatchedNMax];
#pragma unroll
    for (int j = 0; j < kBatchedNMax; ++j) p[j] = j < Model::n ? x[j] : T(0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        T b[NB > 0 ? NB : 1];
        Model::basis(t[i], b);
        const T v = Model::eval(t[i], b, p) - d[i];
        y[i] = w ? w[i] * v : v;
    }
}

}  // namespace mirlsq
