"""Fixed Lanczos runs through the C ABI whose bits the step kernels must keep, written to one .npz -- the child process of
tests/test_gpu_sweep_bits.py and of scripts/record_sweep_bits.py.

    python -m tests.sweep_bits_cases OUT.npz

The library reads EIGENEX_TWO_SWEEPS once per process, so one configuration is one process.  Per case and batch schedule
the file holds alpha, beta, the state fields with the repair counter, and the SHA-256 of the bytes of all basis columns and
of W under "<case>/<schedule>/<key>", and the device's CU count under "cus" (the grid, and with it every partial sum,
follows the CU count).  Importable without a GPU.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import one_sweep_cases as osc  # noqa: E402

# name -> (operator, calls, one workgroup per CU).  Tridiagonal plain CSR, 14 calls: the sweep streams nv = k-1 = 0..11 columns,
# every remainder 0..3 behind none, one and two full groups of four, and k = 0, 1 stream none; rows that end inside, at, one
# behind a 2048-row tile and in a one-row third tile; 513 tiles + 38 rows on one workgroup per CU are three tiles per workgroup
# on 256 CUs (the persistent loop).  laplacian3d(16), 41 calls: row codes, inline finalisers, ten groups per tile.
CASES = {
    "tri63": (("tri", 63), 14, False),
    "tri2048": (("tri", 2048), 14, False),
    "tri2049": (("tri", 2049), 14, False),
    "tri4097": (("tri", 4097), 14, False),
    "tri513tiles": (("tri", 513 * 2048 + 38), 14, True),
    "lap16": (("lap", 16), 41, False),
}
SCHEDULES = ("whole", "mixed")
KEYS = ("alpha", "beta", "state", "sha_V", "sha_W")


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def run_case(ctx, name, out):
    from tests import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    (kind, size), ncalls, per_cu = CASES[name]
    if kind == "lap":
        n = size ** 3
        A = capi.Csr.laplacian3d(ctx, size)
    else:
        n = size
        A = capi.Csr.upload(ctx, n, *osr.tridiagonal_csr(n), column_blocks=0)
    all_schedules = osc.schedules(ncalls)
    for sched in SCHEDULES:
        b = capi.Basis(ctx, A, n, ncalls + 1)
        if per_cu:
            b.tune(1, 4, 0)
        b.upload(capi.VEC_W, osc.start(n))
        for k in all_schedules[sched]:
            b.lanczos_enqueue(k)
        st, alpha, beta = b.lanczos_state()
        key = "%s/%s/" % (name, sched)
        out[key + "alpha"], out[key + "beta"] = alpha, beta
        out[key + "state"] = np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true, b.repairs()], np.int64)
        h = hashlib.sha256()
        for c in range(st.nvec):
            h.update(np.ascontiguousarray(b.download(capi.VEC_COL(c))).tobytes())
        out[key + "sha_V"] = np.frombuffer(h.digest(), np.uint8).copy()
        out[key + "sha_W"] = _sha(b.download(capi.VEC_W))
        b.close()
    A.close()


CONFIGS = (("default", {}), ("two_sweeps", {"EIGENEX_TWO_SWEEPS": "1"}))  # the second: load_w0 in k_dots and k_update


def run_config(name, out_path, timeout=300):
    """one configuration in a child process of its own -> {key: array}; raises RuntimeError if the child did not end normally"""
    import subprocess

    env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
    env.update(dict(CONFIGS)[name])
    try:
        r = subprocess.run([sys.executable, "-m", "tests.sweep_bits_cases", out_path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        raise RuntimeError("%s: timed out\n%s" % (name, (e.stderr or b"")[-4000:]))
    if r.returncode != 0:
        raise RuntimeError("%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-4000:]))
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    import torch

    from cmpt_eigenex_amd import capi

    out = {"cus": np.array(int(torch.cuda.get_device_properties(0).multi_processor_count), np.int64)}
    ctx = capi.Context()
    for name in CASES:
        run_case(ctx, name, out)
    ctx.close()
    tmp = argv[0] + ".part.npz"
    np.savez(tmp, **out)
    os.replace(tmp, argv[0])
    print("%d cases -> %s" % (len(CASES), argv[0]))


if __name__ == "__main__":
    main()
