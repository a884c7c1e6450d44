"""Dense reference of the two k-means operators (xgpr_kmeans_assign_f32, xgpr_kmeans_update_f32, include/xgpr_hip_cluster.h) --
TEST HELPER, numpy only, in ``np.longdouble`` -- with a-priori error caps computed from the inputs, the comparisons the GPU tests
apply to the operators' outputs, and a plain Lloyd loop over them.

Definitions (rows z[n, M] float32 taken as they are, centres c[K, M] float64):

    cn_k = sum_m c[k, m]^2,   s_ik = cn_k - 2 sum_m z[i, m] c[k, m],   labels[i] = min argmin_k s_ik,
    dist2[i] = max(0, sum_m z[i, m]^2 + s_{i, labels[i]})
    sums[k, m] = sum_{i : labels[i] = k} z[i, m],   counts[k] = #{i : labels[i] = k}       (labels outside [0, K) skipped)

Caps, with u = 2^-53 and gamma_j = j u / (1 - j u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: any
order of j float64 operations per result): a float64 operator's s_ik is a sum of M squares and M products (M + 2 roundings deep
at most, the factor 2 being exact), its dist2 one sum deeper, a per-cluster sum ``count`` additions:

    |s_ik error|     <= gamma_{M+2} (cn_k + 2 sum_m |z[i, m]| |c[k, m]|)
    |dist2[i] error| <= gamma_{M+3} (cn_k + 2 sum_m |z[i, m]| |c[k, m]| + sum_m z[i, m]^2)      at k = labels[i]
    |sums[k, m] error| <= gamma_{count_k} sum_{i in k} |z[i, m]|

``gap[i]`` is the distance from the smallest s_ik of row i to the smallest DISTINCT larger one (inf if there is none): identical
centres tie exactly on an operator that runs every column through the same instructions, and do not count.

``mistake=`` plants ONE structural error (sensitivity test only):
    "last_tie"            the HIGHEST index among tied minima wins
    "no_center_norm"      s_ik without cn_k
    "plus_sign"           s_ik = cn_k + 2 z.c
    "sum_all_rows"        every in-range row is added to every cluster's sum
    "count_out_of_range"  labels outside [0, K) are clipped into it and counted
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
MISTAKES = ("last_tie", "no_center_norm", "plus_sign", "sum_all_rows", "count_out_of_range")


def gamma(j):
    j = np.asarray(j, dtype=LD)
    return j * U / (LD(1) - j * U)


def make_case(n, M, K, seed, duplicate=None, spread=1.0):
    """(rows float32 [n, M], centres float64 [K, M]) of seeded Gaussians; ``duplicate=(a, b)`` copies centre a into centre b."""
    rng = np.random.default_rng([n, M, K, seed])
    rows = rng.standard_normal((n, M)).astype(np.float32)
    centers = spread * rng.standard_normal((K, M))
    if duplicate is not None:
        centers[duplicate[1]] = centers[duplicate[0]]
    return rows, centers


class Assign:
    """The dense result of one assign call: s [n, K], labels [n] int32, dist2 [n], gap [n], cap_s [n, K], zz [n] (all longdouble)."""

    def __init__(self, rows, centers, mistake=None):
        assert mistake in (None,) + MISTAKES
        z, c = np.asarray(rows).astype(LD), np.asarray(centers).astype(LD)
        self.n, self.M, self.K = z.shape[0], z.shape[1], c.shape[0]
        cn = (c * c).sum(axis=1)
        dot = z @ c.T
        if mistake == "no_center_norm":
            s = -2 * dot
        elif mistake == "plus_sign":
            s = cn[None, :] + 2 * dot
        else:
            s = cn[None, :] - 2 * dot
        self.s = s
        smin = s.min(axis=1) if self.n else np.zeros(0, dtype=LD)
        hit = s == smin[:, None]
        first = np.argmax(hit, axis=1)
        last = self.K - 1 - np.argmax(hit[:, ::-1], axis=1)
        self.labels = (last if mistake == "last_tie" else first).astype(np.int32)
        self.zz = (z * z).sum(axis=1)
        self.absdot = np.abs(z) @ np.abs(c).T
        self.cap_s = gamma(self.M + 2) * (cn[None, :] + 2 * self.absdot)
        self.cn = cn
        self.dist2 = self.dist2_at(self.labels)
        self.gap = np.where(hit, LD(np.inf), s).min(axis=1) - smin if self.n else np.zeros(0, dtype=LD)

    def dist2_at(self, labels):
        idx = np.arange(self.n)
        return np.maximum(LD(0), self.zz + self.s[idx, labels])

    def cap_dist2_at(self, labels):
        idx = np.arange(self.n)
        return gamma(self.M + 3) * (self.cn[labels] + 2 * self.absdot[idx, labels] + self.zz)

    def excused(self):
        """Rows whose runner-up lies within twice the cap of the minimum: a float64 operator may choose either."""
        idx = np.arange(self.n)
        return self.gap <= 2 * self.cap_s.max(axis=1) if self.n else np.zeros(0, dtype=bool)


def compare_assign(ref, labels, dist2=None):
    """The GPU tests' comparison of an operator's (labels int32 [n], dist2 float64 [n] or None) with the dense ``ref``: -> list of
    problems (empty: passes).  (1) labels in range; (2) the dense s at the chosen label within cap(chosen) + cap(best) of the dense
    minimum -- the operator's own s is within its cap of the dense one at both columns, and it chose its own minimum; (3) every row
    that is not ``excused`` carries the dense label; (4) a row whose chosen s EQUALS the dense minimum exactly (identical centres)
    carries the lowest such index; (5) dist2 within its cap of the dense value at the chosen label."""
    labels = np.asarray(labels)
    bad = []
    if labels.dtype != np.int32 or labels.shape != (ref.n,):
        return [f"labels: dtype {labels.dtype} shape {labels.shape}"]
    if ref.n == 0:
        return bad
    if labels.min() < 0 or labels.max() >= ref.K:
        return [f"labels outside [0, {ref.K}): {labels.min()} .. {labels.max()}"]
    idx = np.arange(ref.n)
    chosen = ref.s[idx, labels]
    best = ref.s[idx, ref.labels]
    slack = ref.cap_s[idx, labels] + ref.cap_s[idx, ref.labels]
    over = chosen - best > slack
    if over.any():
        i = int(np.argmax(over))
        bad.append(f"{int(over.sum())} rows chose a centre beyond the cap, first row {i}: s {float(chosen[i])} against {float(best[i])}")
    wrong = (labels != ref.labels) & ~ref.excused()
    if wrong.any():
        i = int(np.argmax(wrong))
        bad.append(f"{int(wrong.sum())} unexcused rows carry another label, first row {i}: {labels[i]} against {ref.labels[i]}")
    tie = (chosen == best) & (labels != ref.labels)
    if tie.any():
        bad.append(f"{int(tie.sum())} rows chose a higher index among exactly tied centres")
    if dist2 is not None:
        d = np.asarray(dist2)
        if d.dtype != np.float64 or d.shape != (ref.n,):
            return bad + [f"dist2: dtype {d.dtype} shape {d.shape}"]
        err = np.abs(d.astype(LD) - ref.dist2_at(labels))
        cap = ref.cap_dist2_at(labels)
        if not (err <= cap).all():
            i = int(np.argmax(err - cap))
            bad.append(f"dist2 beyond its cap at row {i}: error {float(err[i]):.3e}, cap {float(cap[i]):.3e}")
    return bad


class Update:
    """The dense result of one update call: sums [K, M] longdouble, counts [K] int64, cap [K, M]."""

    def __init__(self, rows, labels, K, mistake=None):
        assert mistake in (None,) + MISTAKES
        z = np.asarray(rows).astype(LD)
        labels = np.asarray(labels).astype(np.int64)
        if mistake == "count_out_of_range":
            counted = np.clip(labels, 0, K - 1)
        else:
            counted = labels
        inside = (labels >= 0) & (labels < K)
        self.K, self.M = K, z.shape[1]
        self.sums = np.zeros((K, self.M), dtype=LD)
        self.cap = np.zeros((K, self.M), dtype=LD)
        self.counts = np.zeros(K, dtype=np.int64)
        for k in range(K):
            members = inside if mistake == "sum_all_rows" else labels == k
            self.sums[k] = z[members].sum(axis=0)
            self.counts[k] = int(((counted == k) & ((counted >= 0) & (counted < K))).sum())
            self.cap[k] = gamma(max(int((labels == k).sum()), 1)) * np.abs(z[labels == k]).sum(axis=0)


def compare_update(ref, sums, counts, extra_cap=None):
    """-> list of problems: counts exact, sums within cap (``extra_cap``: added to it, for results that took additions beyond one
    call's, such as accumulate over two halves), and exact zeros for an empty cluster."""
    sums, counts = np.asarray(sums), np.asarray(counts)
    bad = []
    if sums.dtype != np.float64 or sums.shape != (ref.K, ref.M) or counts.dtype != np.int64 or counts.shape != (ref.K,):
        return [f"sums {sums.dtype} {sums.shape}, counts {counts.dtype} {counts.shape}"]
    if not (counts == ref.counts).all():
        bad.append(f"counts differ: {counts.tolist()} against {ref.counts.tolist()}")
    err = np.abs(sums.astype(LD) - ref.sums)
    cap = ref.cap if extra_cap is None else ref.cap + extra_cap
    if not (err <= cap).all():
        k, m = np.unravel_index(int(np.argmax(err - cap)), err.shape)
        bad.append(f"sums beyond the cap at [{k}, {m}]: error {float(err[k, m]):.3e}, cap {float(cap[k, m]):.3e}")
    empty = ref.counts == 0
    if empty.any() and extra_cap is None and (sums[empty] != 0).any():
        bad.append("an empty cluster's sums are not exactly zero")
    return bad


def lloyd(feats, init, max_iter=100, tol=1e-4, assign=None, update=None):
    """Lloyd's iteration as xgpr_amd.cluster.KernelKMeans runs it, over float64 features in numpy (or over the callables given):
    assign; stop -- centres untouched -- when no label changed or the inertia fell by less than ``tol`` relative; otherwise move
    every non-empty cluster's centre to its mean (an empty one keeps its centre) and count one iteration; after ``max_iter``
    updates one more assign, so that labels and inertia always belong to the returned centres.
    -> (labels int32, centres float64 [K, M], inertia_history list, n_iter, counts int64)."""
    z = np.asarray(feats, dtype=np.float64)
    centers = np.array(init, dtype=np.float64)
    K = centers.shape[0]

    def np_assign(c):
        s = (c * c).sum(axis=1)[None, :] - 2 * z @ c.T
        lab = np.argmin(s, axis=1).astype(np.int32)
        return lab, np.maximum(0, (z * z).sum(axis=1) + s[np.arange(z.shape[0]), lab])

    def np_update(lab):
        sums = np.zeros_like(centers)
        np.add.at(sums, lab, z)
        return sums, np.bincount(lab, minlength=K).astype(np.int64)

    assign = np_assign if assign is None else assign
    update = np_update if update is None else update
    history, n_iter, prev_labels, prev_inertia = [], 0, None, None
    counts = np.zeros(K, dtype=np.int64)
    while True:
        labels, d2 = assign(centers)
        inertia = float(np.sum(d2))
        history.append(inertia)
        if n_iter >= max_iter:
            break
        if prev_labels is not None and ((labels == prev_labels).all() or prev_inertia - inertia < tol * prev_inertia):
            break
        sums, counts = update(labels)
        live = counts > 0
        centers[live] = sums[live] / counts[live, None]
        prev_labels, prev_inertia = labels, inertia
        n_iter += 1
    return labels, centers, history, n_iter, np.bincount(labels, minlength=K).astype(np.int64)
