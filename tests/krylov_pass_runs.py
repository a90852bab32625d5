"""What tests/test_gpu_spin_krylov_passes.py and tests/test_gpu_layout_krylov_passes.py share: the schemes of step calls and the
two runners that make the calls and download the state.  Importable without a GPU; nothing touches the device before a runner is
called.

Schemes, eight calls each (a batch of four or more is captured as a graph):
  a        lanczos_enqueue, default: real handles take the one-sweep step (u_out NULL, scale set), complex ones the two-sweep step
  b_twice  lanczos_enqueue, ORTHO_BATCHED_TWICE   } real handles take the two-sweep step with store_u; no repair and no pending
  b_seq    lanczos_enqueue, ORTHO_SEQUENTIAL      } close show that the one-sweep path was not taken
  c        arnoldi_enqueue, default (no partials)
  d        arnoldi_enqueue, ORTHO_BATCHED_ADAPTIVE (kPassSelfNorm)
  a_split, d_split   a and d as two batches of four
  e_c, e_d complex handles: c and d with the shift 0.3 - 0.2i
a .. d run at shift 0 and -0.37."""
import os

import numpy as np

CALLS = 8
SHIFTS = (0.0, -0.37)
SHIFT_Z = 0.3 - 0.2j

SCHEMES = {  # name -> (lanczos?, ortho mode name, batches, shifts, complex handles only)
    "a": (True, "ORTHO_BATCHED", (CALLS,), SHIFTS, False),
    "b_twice": (True, "ORTHO_BATCHED_TWICE", (CALLS,), SHIFTS, False),
    "b_seq": (True, "ORTHO_SEQUENTIAL", (CALLS,), SHIFTS, False),
    "c": (False, "ORTHO_BATCHED", (CALLS,), SHIFTS, False),
    "d": (False, "ORTHO_BATCHED_ADAPTIVE", (CALLS,), SHIFTS, False),
    "a_split": (True, "ORTHO_BATCHED", (CALLS // 2, CALLS // 2), (-0.37,), False),
    "d_split": (False, "ORTHO_BATCHED_ADAPTIVE", (CALLS // 2, CALLS // 2), (-0.37,), False),
    "e_c": (False, "ORTHO_BATCHED", (CALLS,), (SHIFT_Z,), True),
    "e_d": (False, "ORTHO_BATCHED_ADAPTIVE", (CALLS,), (SHIFT_Z,), True),
}


def state(st):
    return st.nvec, st.iterations, st.stopped


def columns(capi, b, nvec):
    return np.stack([b.download(capi.VEC_COL(c)) for c in range(nvec)]) if nvec else np.zeros((0, b.n_rows), b.dtype)


def two_sweeps_forced():
    return "EIGENEX_TWO_SWEEPS" in os.environ


def _basis(capi, ctx, op, n, x, shift, mode, capacity, big, prepare, interval=1, n_ortho=0, fusion=None):
    b = capi.Basis(ctx, op, n, capacity, n_ortho=n_ortho)
    if big:
        b.tune(2, 1, 0)  # one operator workgroup per CU: the tile loop goes round
    b.configure(shift=shift, interval=interval, ortho_mode=mode)
    if fusion is not None:
        b.set_alpha_fusion(fusion)
    if prepare:
        prepare(b)  # before the start vector goes up: what a test wants in the columns beforehand
    b.upload(capi.VEC_W, x)
    return b


def lanczos(capi, ctx, op, n, x, batches, shift, mode, capacity, big=False, prepare=None, **general):
    """dict(state, alpha, beta, U, repairs, pending) after the batches of lanczos_enqueue calls; pending as the last batch left it.
    general: interval, n_ortho (prepare uploads VEC_ORTHO(q)) and fusion of tests/test_gpu_general_step_passes.py"""
    b = _basis(capi, ctx, op, n, x, shift, mode, capacity, big, prepare, **general)
    for calls in batches:
        b.lanczos_enqueue(calls)
    return lanczos_state(capi, b), b


def lanczos_state(capi, b):
    """the downloaded state of a Lanczos basis, as lanczos() returns it: also between the batches of a test that restarts,
    clones or reserves in between (tests/test_gpu_restart_steps.py)"""
    st, alpha, beta = b.lanczos_state()
    out = dict(state=state(st), lengths=(st.nalpha, st.nbeta), alpha=alpha, beta=beta, pending=b.close_pending(), repairs=b.repairs())
    out["U"] = columns(capi, b, st.nvec)
    return out


def arnoldi(capi, ctx, op, n, x, batches, shift, mode, capacity, big=False, prepare=None, **general):
    b = _basis(capi, ctx, op, n, x, shift, mode, capacity, big, prepare, **general)
    for calls in batches:
        b.arnoldi_enqueue(calls)
    return arnoldi_state(capi, b), b


def arnoldi_state(capi, b):
    st, H = b.arnoldi_projected()
    return dict(state=state(st), lengths=(st.nalpha, st.nbeta), H=H, residue=st.residue, U=columns(capi, b, st.nvec), w=b.download(capi.VEC_W))
