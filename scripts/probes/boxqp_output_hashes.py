"""SHA-256 of what M.solveBoxQPBatched returns (status, iterations, the bytes of x) per order n = 1 .. 16 and precision, for
three cases each on tests/boxqp_cases.family(n, dtype) taken cyclically at count 257: default settings; relTolerance =
absTolerance = 1e-6; the oracle's unconstrained minimisers handed in. Two trees whose kernels compute the same print the same
lines: run it on both and compare the outputs (profiles/r12).
Run from the repository root:  timeout 300 python scripts/probes/boxqp_output_hashes.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mir_optim_amd as M          # noqa: E402
import boxqp_cases as B            # noqa: E402
from oracle import oracle as O     # noqa: E402


def digest(status, x, iterations):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (status, iterations, x))).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "boxqp_output_hashes.txt"))
    out = ap.parse_args().out
    O.build()
    idx = np.arange(257) % B.FAMILY_COUNT
    lines = []
    for n in range(1, 17):
        for dtype in B.DTYPES:
            P, q, l, u = B.family(n, dtype)
            x0 = B.oracle_solve(O, P, q, np.full(n, -np.inf), np.full(n, np.inf), dtype)[1]
            s = M.BoxQPSettings(dtype); s.relTolerance = s.absTolerance = 1e-6
            cases = {"default": {}, "tol 1e-6": {"settings": s}, "x handed in": {"x": x0[idx], "unconstrainedSolution": True}}
            for name, kw in cases.items():
                res = M.solveBoxQPBatched(P[idx], q[idx], l[idx], u[idx], dtype=dtype, **kw)
                lines.append(f"n = {n:2d} {np.dtype(dtype).name} {name:12s} {digest(*res)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)


if __name__ == "__main__":
    main()
