"""Dynamic time warping with a soft minimum, restated in float64 NumPy for one pair: the recursion over the cells in row order, the
gradient as the reverse sweep in closed form, the Viterbi path from hard back-pointers.  What csrc/dtw.hip computes, in the order a
reader would write it down; tests/test_dtw_cpu.py pins it to the goldens of the reference."""
import numpy as np
import torch

STEPS = {   # p -> (steps in candidate order, whether axis steps read the second table)
    0: (((1, 0), (0, 1)), False),
    1: (((1, 0), (0, 1), (1, 1)), False),
    2: (((1, 0), (1, 1)), False),
    3: (((1, 0), (1, 1), (1, 2)), False),
    4: (((1, 0), (0, 1), (1, 1)), True),
    5: (((1, 1), (1, 2), (2, 1)), False),
    6: (((1, 0), (1, 1), (1, 2)), True),
}
METRICS = {"manhattan": 0, "euclidean": 1, "squared-euclidean": 2, "symmetric-kl": 3}
CLIP = 1e-10


def local_distance(x, y, metric):
    """d:(T1, T2) and its derivatives dx, dy:(T1, T2, D) with respect to x_i and y_j"""
    a, b = x[:, None, :], y[None, :, :]
    e = a - b
    if metric == 0:
        return np.abs(e).sum(-1), np.sign(e), -np.sign(e)
    if metric in (1, 2):
        r = np.sqrt((e * e).sum(-1))
        if metric == 2:
            return r * r, 2 * e, -2 * e
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.where(r[..., None] == 0, 0.0, e / r[..., None])
        return r, g, -g
    q1, q2 = a / b, b / a
    in1, in2 = q1 >= CLIP, q2 >= CLIP   # a clipped quotient passes no derivative
    d = (a * np.log(np.maximum(q1, CLIP))).sum(-1) + (b * np.log(np.maximum(q2, CLIP))).sum(-1)
    dx = np.log(np.maximum(q1, CLIP)) + in1 - np.where(in2, q2, 0.0)
    dy = np.log(np.maximum(q2, CLIP)) + in2 - np.where(in1, q1, 0.0)
    return d, dx, dy


def softmin(c, gamma):
    m = min(c)
    return m - gamma * np.log(sum(np.exp(-(v - m) / gamma) for v in c))


def dtw(x, y, metric=1, p=4, gamma=1e-3, lengths=None, gdistance=1.0):
    """x:(T1, D), y:(T2, D) float64 -> dict(distance, gx, gy, path:(T, 2) int64, margin: the smallest gap between the winning candidate
    and the runner-up over the cells of the path -- inf where no cell had a choice)."""
    metric = METRICS.get(metric, metric)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    T1, T2 = len(x), len(y)
    n1, n2 = (T1, T2) if lengths is None else (int(lengths[0]), int(lengths[1]))
    steps, two = STEPS[p]
    d, ddx, ddy = local_distance(x, y, metric)
    inf = np.inf
    R, R2 = np.full((T1, T2), inf), np.full((T1, T2), inf)
    R[0, 0] = d[0, 0]

    def candidates(i, j):
        """[(k, candidate, reads the second table, counts for the second table)] of the steps whose source is inside and finite"""
        out = []
        for k, (a, b) in enumerate(steps):
            if i - a < 0 or j - b < 0:
                continue
            axis = two and (a == 0 or b == 0)
            v = (R2 if axis else R)[i - a, j - b]
            if v != inf:
                out.append((k, (a + b) * d[i, j] + v, axis, two and not axis))
        return out

    for i in range(n1):
        for j in range(n2):
            c = candidates(i, j)
            if c:
                R[i, j] = softmin([v for _, v, _, _ in c], gamma)
            c2 = [v for _, v, _, second in c if second]
            if c2:
                R2[i, j] = softmin(c2, gamma)
    total = n1 + n2
    distance = R[n1 - 1, n2 - 1] / total

    # the reverse sweep: G, G2 the adjoints of R, R2
    G, G2 = np.zeros((T1, T2)), np.zeros((T1, T2))
    gD = np.zeros((T1, T2))
    if R[n1 - 1, n2 - 1] != inf:
        G[n1 - 1, n2 - 1] = gdistance / total
    for i in range(n1 - 1, -1, -1):
        for j in range(n2 - 1, -1, -1):
            if G[i, j] == 0 and G2[i, j] == 0:
                continue
            if i == 0 and j == 0:
                gD[0, 0] = G[0, 0]
                continue
            for k, v, axis, second in candidates(i, j):
                a, b = steps[k]
                msg = G[i, j] * np.exp(-(v - R[i, j]) / gamma)
                if second and G2[i, j] != 0:
                    msg += G2[i, j] * np.exp(-(v - R2[i, j]) / gamma)
                (G2 if axis else G)[i - a, j - b] += msg
                gD[i, j] += msg * (a + b)
    gx = np.einsum("ij,ijk->ik", gD, ddx)
    gy = np.einsum("ij,ijk->jk", gD, ddy)

    # the path: the hard argmin of each cell, the first of equal candidates; after a move that kept a coordinate, the second table's
    i, j, second, margin = n1 - 1, n2 - 1, False, inf
    path = [(i, j)]
    while i > 0 or j > 0:
        c = [(v, k) for k, v, axis, _ in candidates(i, j) if not (second and axis)]
        if not c:
            break
        best = min(c)   # (value, step index): ties go to the first step
        if len(c) > 1:
            margin = min(margin, sorted(v for v, _ in c)[1] - best[0])
        a, b = steps[best[1]]
        i, j = i - a, j - b
        second = two and (a == 0 or b == 0)
        path.append((i, j))
    return {"distance": distance, "gx": gx, "gy": gy, "path": np.array(path[::-1], np.int64), "margin": margin, "end": R[n1 - 1, n2 - 1]}


def golden_cases(directory):
    """the cases of tests/golden/dtw.npz + dtw_api.json (make_golden_dtw.py) as dicts: the options and, in float64, x, y, gx, gy (2-D),
    distance, e_ref, e_gref, path"""
    import json
    import os

    data = np.load(os.path.join(directory, "dtw.npz"))
    out = []
    for n, c in enumerate(json.load(open(os.path.join(directory, "dtw_api.json")))["cases"]):
        D = max(c["D"], 1)   # D = 0 marks (T,) inputs: one column here
        flat, nx, ny = data[f"c{n}"], c["T1"] * D, c["T2"] * D
        assert len(flat) == 2 * (nx + ny) + 3
        x, y, gx, gy = flat[:nx], flat[nx:nx + ny], flat[nx + ny:2 * nx + ny], flat[2 * nx + ny:2 * (nx + ny)]
        out.append(dict(c, n=n, x=x.reshape(-1, D), y=y.reshape(-1, D), gx=gx.reshape(-1, D), gy=gy.reshape(-1, D), distance=flat[-3],
                        e_ref=flat[-2], e_gref=flat[-1], path=data[f"p{n}"], metric_code=METRICS[c["metric"]]))
    return out


def case_id(c):
    return f"{c['n']}-p{c['p']}-{c['metric']}-g{c['gamma']}-{c['T1']}x{c['T2']}x{c['D']}" + ("-len" if c["lengths"] else "")


ERRORS = {   # name -> a call on the package `m` that must raise: make_golden_dtw.py records what the reference raises, test_dtw_cpu.py compares
    "bad metric": lambda m: m.DynamicTimeWarping(metric="chebyshev"),
    "bad metric code": lambda m: m.DynamicTimeWarping(metric=4),
    "bad p": lambda m: m.DynamicTimeWarping(p=7),
    "softness zero": lambda m: m.DynamicTimeWarping(softness=0),
    "softness negative": lambda m: m.functional.dtw(torch.zeros(3), torch.zeros(3), softness=-1.0),
    "4-D input": lambda m: m.DynamicTimeWarping()(torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 3, 2)),
    "x 3-D, y 2-D": lambda m: m.DynamicTimeWarping()(torch.zeros(1, 3, 2), torch.zeros(3, 2)),
    "mismatched dims": lambda m: m.DynamicTimeWarping()(torch.zeros(3, 2), torch.zeros(4, 3)),
    "1-D lengths": lambda m: m.DynamicTimeWarping()(torch.zeros(1, 3, 2), torch.zeros(1, 4, 2), torch.tensor([3, 4])),
    "merge: 1-D indices": lambda m: m.DynamicTimeWarping.merge(torch.zeros(3), torch.zeros(4), torch.zeros(5, dtype=torch.long)),
    "merge: three columns": lambda m: m.functional.dtw_merge(torch.zeros(3), torch.zeros(4), torch.zeros(5, 3, dtype=torch.long)),
    "merge: x 1-D, y 2-D": lambda m: m.functional.dtw_merge(torch.zeros(3), torch.zeros(4, 1), torch.zeros(5, 2, dtype=torch.long)),
}
