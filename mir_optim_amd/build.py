"""Build the HIP libraries in-tree with hipcc for gfx950 (cross-compiles without a GPU).

  lib/libmir_optim_amd.so            the solver + C ABI (include/mir_optim_amd.h)
  lib/libmir_optim_amd_workloads.so  device residual callbacks of the synthetic workloads

The solver is a dozen translation units (csrc/driver.h lists them): each is compiled to an object of its own under
build/obj/ -- in parallel, and only when it or one of the headers IT includes (the compiler's own dependency file, -MMD)
is newer -- and the objects are linked. A kernel edit costs the translation units that include that kernel's header
(usually one launch_*.hip), not the library.
"""
import functools
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(HERE, "build", "obj")
SOLVER_LIB = os.path.join(LIBDIR, "libmir_optim_amd.so")
WORKLOADS_LIB = os.path.join(LIBDIR, "libmir_optim_amd_workloads.so")

SOLVER_UNITS = ["abi.hip", "workspace.hip", "solver_loop.hip", "solver_jacobian.hip", "launch_jtj.hip", "launch_broyden.hip",
                "launch_solve_d.hip", "launch_solve_s.hip", "batched.hip", "batched_d.hip", "comm.hip", "unit_entries.hip", "covariance.hip",
                "launch_spd_inverse.hip", "launch_boxqp.hip", "launch_boxqp16_s.hip", "launch_boxqp16_d.hip", "launch_boxqp64_s.hip",
                "launch_boxqp64_d.hip", "batched_bounded.hip", "batched_bounded_d.hip", "batched16_d.hip", "batched16_ex_d.hip",
                "fit_spline.cpp", "fit_spline_gpu.hip", "batched_predict.hip", "batched_predict_d.hip"]
WORKLOAD_UNITS = ["workloads.hip", "workloads_gemm.hip", "workloads_resident.hip"]

_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + os.environ.get("MIR_OPTIM_AMD_CXXFLAGS", "").split()


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build the gfx950 kernels")
    return exe


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any((not os.path.exists(s)) or os.path.getmtime(s) > t for s in sources)


def _deps(d, base=""):
    """The files an object or library was compiled from, as the compiler recorded them (`-MMD -MF d`): the translation unit and
    exactly the headers it includes -- an edit of a kernel header recompiles what includes it and nothing else. None: no record.
    base: the directory the compiler ran in, for the relative paths of the record."""
    if not os.path.exists(d):
        return None
    toks = open(d).read().replace("\\\n", " ").split()
    return [os.path.join(base, t) for t in toks[1:] if not t.endswith(":") and not t.startswith("/opt/") and not t.startswith("/usr/")]


def _run(cmd, verbose, cwd=None):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=cwd)


def _compile_units(units, extra, force, verbose, jobs):
    objs, todo = [], []
    for u in units:
        src = os.path.join(CSRC, u)
        obj = os.path.join(OBJDIR, os.path.splitext(u)[0] + ".o")
        objs.append(obj)
        deps = _deps(obj[:-2] + ".d")
        if force or deps is None or _stale(obj, [src] + deps):
            todo.append([_hipcc()] + _FLAGS + extra + ["-MMD", "-MF", obj[:-2] + ".d", "-c", src, "-o", obj])
    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda c: _run(c, verbose), todo))
    return objs, bool(todo)


def build(force=False, verbose=False, jobs=None):
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(OBJDIR, exist_ok=True)
    # the flags are part of what an object depends on (a profiling build must not reuse the product objects)
    stamp = os.path.join(OBJDIR, "flags.txt")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(_FLAGS):
        force = True
    objs, rebuilt = _compile_units(SOLVER_UNITS, [], force, verbose, jobs)
    open(stamp, "w").write(" ".join(_FLAGS))
    # the link takes the same flags as the compilations (-g, sanitizer or profiling flags from MIR_OPTIM_AMD_CXXFLAGS reach the .so)
    if force or rebuilt or _stale(SOLVER_LIB, objs):
        _run([_hipcc()] + _FLAGS + ["-shared", "-o", SOLVER_LIB] + objs + ["-ldl"], verbose)
    # the caller side: residual kernels of the synthetic workloads (the C entries + small kernels, the batched GEMM, and the
    # resident models, which are compiled against the device header of the resident-J solver like a caller's own model would be)
    wobjs, wrebuilt = _compile_units(WORKLOAD_UNITS, ["-fopenmp"], force, verbose, 3)     # OpenMP: host-side data generation / host residual
    if force or wrebuilt or _stale(WORKLOADS_LIB, wobjs):
        _run([_hipcc()] + _FLAGS + ["-shared", "-fopenmp", "-o", WORKLOADS_LIB] + wobjs, verbose)
    return SOLVER_LIB, WORKLOADS_LIB


if __name__ == "__main__":
    build(force=True, verbose=True)


# tests/user_model/<name>.hip: a caller's own residual models, each compiled into tests/user_model/lib<name>.so
USER_MODEL_DIR = os.path.join(os.path.dirname(HERE), "tests", "user_model")
USER_MODELS = [
    "user_model",                 # float models on the batched path and one on the resident-J path
    "user_model_f64",             # a double model on the batched path
    "user_model_weighted",        # a weighted fit with covariance
    "user_model_bounded",         # a fit with binding bounds
    "user_model_n16",             # models of 9 and 13 parameters on the batched path
    "user_model_n16_weighted",    # their weighted fits with covariance
    "user_model_problem_bounds",  # a fit with a box per problem
    "user_model_predict",         # fitted curves and their confidence bands
]


def example_paths(name):
    """(source, library) of the example tests/user_model/<name>.hip"""
    return os.path.join(USER_MODEL_DIR, name + ".hip"), os.path.join(USER_MODEL_DIR, "lib" + name + ".so")


def build_user_model_example(force=False, verbose=False):
    """tests/user_model/: a caller's own residual models compiled against the public device headers (include/) into libraries of
    their own, one per source of USER_MODELS -- what a user of those headers does. Built here so that they travel prebuilt. A
    library is rebuilt when its source or a header it includes (the compiler's own dependency file, as for the solver's units)
    is newer. The compiler runs in the repository's root on relative paths, so that the record holds for the tree wherever it
    lies. Returns the path of libuser_model.so."""
    root = os.path.dirname(HERE)
    os.makedirs(OBJDIR, exist_ok=True)
    for name in USER_MODELS:
        src, out = example_paths(name)
        dep = os.path.join(OBJDIR, name + ".d")
        deps = _deps(dep, root)
        if force or deps is None or _stale(out, [src] + deps):
            _run([_hipcc()] + _FLAGS + ["-shared", "-I", "include", "-MMD", "-MF", dep, "-o", out, os.path.relpath(src, root)], verbose,
                 cwd=root)
    return example_paths("user_model")[1]


def example_lib(name, force=False, verbose=False):
    """Builds (when stale) and returns the path of tests/user_model/lib<name>.so."""
    build_user_model_example(force=force, verbose=verbose)
    return example_paths(name)[1]


# user_model_f64_paths(), user_model_f64_lib(force=False, verbose=False), ...: the two functions above for each example by name
for _name in USER_MODELS:
    globals()[_name + "_paths"] = functools.partial(example_paths, _name)
    globals()[_name + "_lib"] = functools.partial(example_lib, _name)
