"""The checker of the k-medoid reduction of joint samples to scene modes
(include/g2k_scene_modes.h): the definition restated in float64 NumPy on the
float32 draws.  Per scored scene-frame (P >= 1) the K + 1 items (the K joint
draws, then the targets), each P x 12 x 2, their matrix A of summed per-step
displacements, the clustering on it (PAM BUILD, the alternating rounds, the
final assignment) and the modes' scores.  Both sides are double, so A differs
by summation order alone (NumPy has no fma: dy dy + dx dx is rounded twice,
one more last-bit difference per term); the clustering is integer decisions on
A, which a last-bit difference can move only where the two best candidates of
an argmin or argmax are closer than ``MARGIN`` relative without being
bit-equal: the checker counts those per scene-frame (``ambiguous``), and the
sums of every decision run in ascending index (cumulative sums, not NumPy's
pairwise ones), so that the exact ties of the definition are exact here too.
``scene_modes_ref`` takes [K, S, F, 24, N] draws (the device's own, or the
restated samplers').  Test helper, not a test module."""
import numpy as np

L = 12
M_MAX, K_MIN, K_MAX, ITERS_MAX = 32, 2, 64, 32
MARGIN = 1e-9


def band_to_steps(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, L, 2]."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    return np.moveaxis(xy, -3, -2)                                  # [..., N, L, 2]


def seq_sum(a, axis=-1):
    """The sum along ``axis`` in ascending index from 0 (np.sum adds pairwise)."""
    a = np.asarray(a, np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def frame_matrix(Z):
    """Z [K + 1, P, L, 2] float64 items (the last the targets) -> (A [K + 1, K +
    1], Fn [K], Mx [K])."""
    d = Z[:, None] - Z[None]                                         # [NI, NI, P, L, 2]
    e = np.sqrt(d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])       # [NI, NI, P, L]
    A = seq_sum(e.reshape(e.shape[0], e.shape[1], -1))               # members, then steps
    last = e[:-1, -1, :, L - 1]                                      # [K, P]: draw k against the targets
    return A, seq_sum(last), last.max(axis=1)


class _Near:
    """Counts the decisions whose two best candidates are closer than MARGIN
    relative without being bit-equal."""
    def __init__(self, margin):
        self.margin, self.n, self.decisions = margin, 0, 0

    def best(self, v, want_max=False):
        """The index of the best of v (the lowest on an exact tie)."""
        v = np.asarray(v, np.float64)
        i = int(np.argmax(v) if want_max else np.argmin(v))
        self.decisions += 1
        if len(v) > 1:
            rest = np.delete(v, i)
            rest = rest[rest != v[i]]
            if len(rest):
                o = rest.max() if want_max else rest.min()
                if abs(o - v[i]) <= self.margin * max(abs(o), abs(v[i])):
                    self.n += 1
        return i


def cluster(A, K, M, iters, near=None):
    """A [>= K, >= K] -> dict(med [M], asg [K], counts [M], rounds, moved: the
    rounds that changed a medoid): the header's clustering."""
    near = near or _Near(MARGIN)
    D = np.asarray(A, np.float64)[:K, :K]
    med = [near.best(seq_sum(D, axis=1))]
    dmin = D[:, med[0]].copy()
    for _ in range(1, M):
        gain = seq_sum(np.maximum(0.0, dmin[None, :] - D), axis=1)
        free = np.array([j for j in range(K) if j not in med])
        med.append(int(free[near.best(gain[free], want_max=True)]))
        dmin = np.minimum(dmin, D[:, med[-1]])
    med = np.array(med)

    def assign():
        return np.array([near.best(D[k, med]) for k in range(K)])
    rounds = moved = 0
    for _ in range(iters):
        a = assign()
        changed = False
        for m in range(M):
            mem = np.flatnonzero(a == m)
            if len(mem) == 0:
                continue
            j = int(mem[near.best(seq_sum(D[np.ix_(mem, mem)], axis=1))])
            if j != med[m]:
                med[m], changed = j, True
        rounds += 1
        if not changed:
            break
        moved += 1
    a = assign()
    return dict(med=med, asg=a, counts=np.bincount(a, minlength=M), rounds=rounds, moved=moved)


def frame_modes(Z, K, M, iters, near=None):
    """One scored scene-frame from its items Z [K + 1, P, L, 2] float64 ->
    dict(i [4]: P, mA, mF, rounds; d [8]: cA, cF, w_mA, w_mF, cost, raw, all,
    mx; med [M]; counts [M]; moved)."""
    near = near or _Near(MARGIN)
    P = Z.shape[1]
    A, Fn, Mx = frame_matrix(Z)
    c = cluster(A, K, M, iters, near)
    med, cnt = c["med"], c["counts"]
    mA = near.best(A[med, K])
    mF = near.best(Fn[med])
    cost = seq_sum(A[np.arange(K), med[c["asg"]]]) / float(12 * K * P)
    d = [A[med[mA], K] / float(12 * P), Fn[med[mF]] / float(P), cnt[mA] / float(K), cnt[mF] / float(K), cost,
         A[:M, K].min() / float(12 * P), A[:K, K].min() / float(12 * P), Mx[med].min()]
    return dict(i=[P, mA, mF, c["rounds"]], d=d, med=med, counts=cnt, moved=c["moved"])


def scene_modes_ref(draws, targets, members, K, M, iters, miss_radius, margin=MARGIN):
    """draws [K, S, F, 24, N] float32, targets [S, F or 1, N, L, 2], members [S,
    F, N] bool -> dict(per_frame_i [S, F, 4] int64, per_frame_d [S, F, 8]
    float64, medoids, counts [S, F, M] int64, sums [S, 8], tot [S, 4] int64,
    ambiguous [S, F] bool: a decision of the scene-frame within ``margin``,
    moved [S, F]: the rounds that changed a medoid, frames: the scored ones)."""
    draws = np.asarray(draws)
    assert draws.dtype == np.float32 and draws.shape[0] == K
    S, F, N = members.shape
    x = band_to_steps(draws)                                           # [K, S, F, N, L, 2]
    y = np.broadcast_to(np.asarray(targets, np.float32), (S, F, N, L, 2))
    pi = np.zeros((S, F, 4), np.int64)
    pd = np.zeros((S, F, 8), np.float64)
    med = np.zeros((S, F, M), np.int64)
    cnt = np.zeros((S, F, M), np.int64)
    amb = np.zeros((S, F), bool)
    moved = np.zeros((S, F), np.int64)
    sums = np.zeros((S, 8), np.float64)
    tot = np.zeros((S, 4), np.int64)
    r32 = float(np.float32(miss_radius))
    for s in range(S):
        for f in range(F):
            idx = np.flatnonzero(members[s, f])
            P = len(idx)
            if P < 1:
                continue
            Z = np.concatenate([x[:, s, f, idx], y[None, s, f, idx]]).astype(np.float64)
            near = _Near(margin)
            r = frame_modes(Z, K, M, iters, near)
            pi[s, f], pd[s, f], med[s, f], cnt[s, f] = r["i"], r["d"], r["med"], r["counts"]
            amb[s, f], moved[s, f] = near.n > 0, r["moved"]
            d = pd[s, f]
            sums[s] = sums[s] + [P * d[0], P * d[1], (1.0 - d[2]) * (1.0 - d[2]), (1.0 - d[3]) * (1.0 - d[3]),
                                 P * d[4], P * d[5], P * d[6], 0.0]
            tot[s] += [1, P, int(d[7] > r32), r["i"][3]]
    return dict(per_frame_i=pi, per_frame_d=pd, medoids=med, counts=cnt, sums=sums, tot=tot, ambiguous=amb,
                moved=moved, frames=int(tot[:, 0].sum()))


def figures(sums, tot):
    """dict(frames, jade, jfde, brier_jade, brier_jfde, miss_rate, cost,
    raw_jade, all_jade, rounds) from the outputs summed over the scenes."""
    s = np.asarray(sums, np.float64).sum(axis=0)
    t = np.asarray(tot, np.int64).sum(axis=0)
    n, p = int(t[0]), int(t[1])
    nan = float("nan")
    per = lambda v, k: v / k if k else nan
    return dict(frames=n, jade=per(s[0], p), jfde=per(s[1], p), brier_jade=per(s[0], p) + per(s[2], n),
                brier_jfde=per(s[1], p) + per(s[3], n), miss_rate=per(float(t[2]), n), cost=per(s[4], p),
                raw_jade=per(s[5], p), all_jade=per(s[6], p), rounds=per(float(t[3]), n))


# ---------------------------------------------------------------------------
# the definition once more, by plain Python loops
# ---------------------------------------------------------------------------
def frame_loops(Z, K, M, iters):
    """``frame_modes`` by plain loops in the header's order -> (i [4], d [8],
    med [M], counts [M])."""
    NI, P = len(Z), len(Z[0])
    A = [[0.0] * NI for _ in range(NI)]
    Fn, Mx = [0.0] * K, [0.0] * K
    for j in range(NI):
        for l in range(j + 1, NI):
            acc = 0.0
            for i in range(P):
                for t in range(L):
                    dx = float(Z[j][i][t][0]) - float(Z[l][i][t][0])
                    dy = float(Z[j][i][t][1]) - float(Z[l][i][t][1])
                    e = (dy * dy + dx * dx) ** 0.5
                    acc += e
                    if l == NI - 1 and t == L - 1:
                        Fn[j] += e
                        Mx[j] = max(Mx[j], e)
            A[j][l] = A[l][j] = acc

    def argbest(vals, better):
        b = 0
        for i in range(1, len(vals)):
            if better(vals[i], vals[b]):
                b = i
        return b
    lt, gt = (lambda a, b: a < b), (lambda a, b: a > b)

    def rowsum(j, ks):
        acc = 0.0
        for k in ks:
            acc += A[j][k]
        return acc
    med = [argbest([rowsum(j, range(K)) for j in range(K)], lt)]
    dmin = [A[k][med[0]] for k in range(K)]
    for _ in range(1, M):
        free = [j for j in range(K) if j not in med]
        gains = []
        for j in free:
            acc = 0.0
            for k in range(K):
                acc += max(0.0, dmin[k] - A[j][k])
            gains.append(acc)
        med.append(free[argbest(gains, gt)])
        dmin = [min(dmin[k], A[k][med[-1]]) for k in range(K)]
    assign = lambda: [argbest([A[k][b] for b in med], lt) for k in range(K)]
    rounds = 0
    for _ in range(iters):
        a = assign()
        changed = False
        for m in range(M):
            mem = [k for k in range(K) if a[k] == m]
            if not mem:
                continue
            j = mem[argbest([rowsum(j, mem) for j in mem], lt)]
            if j != med[m]:
                med[m], changed = j, True
        rounds += 1
        if not changed:
            break
    a = assign()
    cnt = [a.count(m) for m in range(M)]
    mA = argbest([A[b][K] for b in med], lt)
    mF = argbest([Fn[b] for b in med], lt)
    cost = 0.0
    for k in range(K):
        cost += A[k][med[a[k]]]
    d = [A[med[mA]][K] / (12 * P), Fn[med[mF]] / P, cnt[mA] / K, cnt[mF] / K, cost / (12 * K * P),
         min(A[k][K] for k in range(M)) / (12 * P), min(A[k][K] for k in range(K)) / (12 * P),
         min(Mx[b] for b in med)]
    return [P, mA, mF, rounds], d, med, cnt
