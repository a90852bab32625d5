"""numpy restatement of the finite-temperature Lanczos method and the dense answers it is held against, for
tests/test_gpu_thermal_lanczos.py: the sector Hamiltonian and the correlation operators as dense matrices (from the states by
enumeration, tests/spin_sector_reference.py), exact thermal averages by numpy.linalg.eigh, the +-1 start vectors of
eigenex_vec_random_signs from the hash that include/eigenex_hip.h states, a Lanczos run with full re-orthogonalisation, the
sums and the delete-one jackknife.  Nothing here uses the library's thermal code.

    python tests/thermal_reference.py        the statistical case of the GPU test on the CPU, for the seed the test names
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_sector_reference as ss  # noqa: E402

G = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def _mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sign_vector(n, seed, stream):
    """eigenex_vec_random_signs: key = mix((mix(seed + G) ^ stream) + G), h = mix((key ^ row) + G), -1 where bit 63 of h is set"""
    key = _mix((_mix(seed + G) ^ stream) + G)
    return np.array([-1.0 if _mix((key ^ r) + G) >> 63 else 1.0 for r in range(n)])


def sector_matrices(L, n_up, bonds):
    """(H, zz, xy): the dense Hamiltonian of the sector and, per pair (i, j), i < j, Sz_i Sz_j as a diagonal (a vector) and
    Sx_i Sx_j + Sy_i Sy_j as a matrix"""
    st = ss.states(L, n_up)
    n = st.size
    sig = np.array([2.0 * ((st >> np.uint64(i)) & np.uint64(1)).astype(np.float64) - 1 for i in range(L)])
    zz, xy = {}, {}
    for i in range(L):
        for j in range(i + 1, L):
            zz[i, j] = sig[i] * sig[j] / 4
            A = np.zeros((n, n))
            on = np.flatnonzero(sig[i] != sig[j])
            A[on, ss.rank(st, st[on] ^ np.uint64((1 << i) | (1 << j)))] = 0.5
            xy[i, j] = A
    H = np.zeros((n, n))
    for (i, j, jz, jxy) in bonds:
        a, b = min(i, j), max(i, j)
        H += np.diag(jz * zz[a, b]) + jxy * xy[a, b]
    return H, zz, xy


def exact(E, betas, diag_of=None):
    """dense answers from the eigenvalues E (and, per observable, its diagonal in the eigenbasis): dict beta -> (logZ, E, C, S, [<A>])"""
    out = {}
    for b in betas:
        w = np.exp(-b * (E - E.min()))
        Z = w.sum()
        e = (w * E).sum() / Z
        c = b * b * ((w * (E - e) ** 2).sum() / Z)
        logz = np.log(Z) - b * E.min()
        out[b] = (logz, e, c, b * e + logz, [] if diag_of is None else [(w * d).sum() / Z for d in diag_of])
    return out


def lanczos_sample(H, v, M, ops, threshold=1e-12):
    """(theta, w, a[t]) of one run from v: full re-orthogonalisation (twice), breakdown at beta <= threshold"""
    v = v / np.linalg.norm(v)
    V, alpha, beta = [v], [], []
    for k in range(M):
        w = H @ V[k]
        alpha.append(V[k] @ w)
        if k == M - 1:
            break
        for _ in range(2):
            w -= np.array(V).T @ (np.array(V) @ w)
        b = np.linalg.norm(w)
        if b <= threshold:
            break
        beta.append(b)
        V.append(w / b)
    n = len(alpha)
    T = np.diag(alpha) + np.diag(beta[: n - 1], 1) + np.diag(beta[: n - 1], -1)
    theta, S = np.linalg.eigh(T)
    Vm = np.array(V[:n])
    a = [S[0] * (S.T @ (Vm @ (op * V[0] if op.ndim == 1 else op @ V[0]))) for op in ops]
    return theta, S[0] ** 2, a


def sums(samples, N, beta, skip=None):
    """(logZ, E, C, S, [<A_t>]) over the samples but `skip`"""
    use = [s for r, s in enumerate(samples) if r != skip]
    e0 = min(s[0].min() for s in use)
    m0 = sum((s[1] * np.exp(-beta * (s[0] - e0))).sum() for s in use)
    m1 = sum((s[1] * (s[0] - e0) * np.exp(-beta * (s[0] - e0))).sum() for s in use)
    var = sum((s[1] * (s[0] - e0 - m1 / m0) ** 2 * np.exp(-beta * (s[0] - e0))).sum() for s in use)
    logz = np.log(N / len(use)) + np.log(m0) - beta * e0
    e = e0 + m1 / m0
    obs = [sum((s[2][t] * np.exp(-beta * (s[0] - e0))).sum() for s in use) / m0 for t in range(len(use[0][2]))]
    return logz, e, beta * beta * var / m0, beta * e + logz, obs


def flat(x):
    return np.array(list(x[:4]) + list(x[4]))


def jackknife(samples, N, beta):
    R = len(samples)
    f = np.array([flat(sums(samples, N, beta, skip=i)) for i in range(R)])
    return np.sqrt((R - 1) / R * ((f - f.mean(axis=0)) ** 2).sum(axis=0))


# the statistical case: sector (12,6) of the ring with Jz = 1, Jxy = 0.7, R = 40 sign vectors, M = 50
STAT = dict(L=12, n_up=6, jz=1.0, jxy=0.7, R=40, M=50, betas=(0.1, 0.5, 1.0, 2.0), seed=20260, first_stream=0)


def stat_case(seed=None):
    """the worst |FTLM - dense| / jackknife error over log Z, E, C, S and the 12 nearest-neighbour ZZ and XY correlations and all
    betas, in numpy, with the device's sign vectors"""
    c = STAT
    L = c["L"]
    bonds = [(i, (i + 1) % L, c["jz"], c["jxy"]) for i in range(L)]
    H, zz, xy = sector_matrices(L, c["n_up"], bonds)
    nn = [(min(i, (i + 1) % L), max(i, (i + 1) % L)) for i in range(L)]
    ops = [zz[p] for p in nn] + [xy[p] for p in nn]
    E, U = np.linalg.eigh(H)
    diag_of = [(U * (op[:, None] * U if op.ndim == 1 else op @ U)).sum(axis=0) for op in ops]
    ex = exact(E, c["betas"], diag_of)
    n = H.shape[0]
    samples = [lanczos_sample(H, sign_vector(n, c["seed"] if seed is None else seed, c["first_stream"] + r), c["M"], ops) for r in range(c["R"])]
    worst = 0.0
    for b in c["betas"]:
        got, err = flat(sums(samples, n, b)), jackknife(samples, n, b)
        worst = max(worst, float(np.abs((got - flat(ex[b])) / err).max()))
    return worst


if __name__ == "__main__":
    print("seed %d: worst deviation = %.2f standard errors" % (STAT["seed"], stat_case()))
