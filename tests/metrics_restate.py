"""Plain numpy float64 restatement of the objective-evaluation kernels (csrc/metrics.hip, include/ctts.h): the mel cepstrum, the local
cost, the DTW recurrence with the stated tie rule, the backtrack and the path sums.  Written from the definitions; the yardstick of
tests/test_metrics_gpu.py, pinned by tests/test_metrics_restate_cpu.py."""
import numpy as np

MCD_DB = 10.0 * np.sqrt(2.0) / np.log(10.0)
STEPS = ((1, 1), (1, 0), (0, 1))          # direction 0, 1, 2: diagonal, (i-1, j), (i, j-1)


def dct_matrix(M, K):
    """[K, M]: row k-1 = sqrt(2/M) cos(pi k (m + 1/2) / M), k = 1 .. K"""
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / M) * np.cos(np.pi * k * (m + 0.5) / M)


def mel_cepstrum(mel, K=13):
    """mel [M, F] -> [F, K]"""
    mel = np.asarray(mel, dtype=np.float64)
    return (dct_matrix(mel.shape[0], K) @ mel).T


def local_cost(x, y):
    """x [Lx, K], y [Ly, K] -> d [Lx, Ly] = ||x_i - y_j||_2"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))


def accumulate(d):
    """A(i,j) = d(i,j) + min(A(i-1,j-1), A(i-1,j), A(i,j-1)), A(0,0) = d(0,0); also the direction of every cell: the diagonal wins when
    it is <= both others, then (i-1,j), then (i,j-1)"""
    Lx, Ly = d.shape
    A = np.full((Lx, Ly), np.inf)
    dirs = np.zeros((Lx, Ly), dtype=np.int8)
    for i in range(Lx):
        for j in range(Ly):
            if i == 0 and j == 0:
                A[0, 0] = d[0, 0]
                continue
            diag = A[i - 1, j - 1] if i > 0 and j > 0 else np.inf
            up = A[i - 1, j] if i > 0 else np.inf
            left = A[i, j - 1] if j > 0 else np.inf
            best, k = diag, 0
            if up < best:
                best, k = up, 1
            if left < best:
                best, k = left, 2
            A[i, j] = d[i, j] + best
            dirs[i, j] = k
    return A, dirs


def accumulate_fast(d):
    """the same A (no directions) one anti-diagonal at a time: for the large case of the GPU test"""
    Lx, Ly = d.shape
    A = np.full((Lx + 1, Ly + 1), np.inf)
    A[0, 0] = 0.0
    for s in range(Lx + Ly - 1):
        i = np.arange(max(0, s - Ly + 1), min(s, Lx - 1) + 1)
        j = s - i
        A[i + 1, j + 1] = d[i, j] + np.minimum(A[i, j], np.minimum(A[i, j + 1], A[i + 1, j]))
    return A[1:, 1:]


def backtrack(dirs):
    i, j = dirs.shape[0] - 1, dirs.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        di, dj = STEPS[dirs[i, j]]
        i, j = i - di, j - dj
        path.append((i, j))
    return path[::-1]


def dtw(x, y):
    """-> (cost, path as a list of (i, j)); empty input: (0.0, [])"""
    if len(x) == 0 or len(y) == 0:
        return 0.0, []
    A, dirs = accumulate(local_cost(x, y))
    return float(A[-1, -1]), backtrack(dirs)


def path_cost(d, path):
    return float(sum(d[i, j] for i, j in path))


def monotone_paths(Lx, Ly):
    """every path from (0,0) to (Lx-1, Ly-1) with steps (1,1), (1,0), (0,1)"""
    out = []

    def walk(i, j, acc):
        acc = acc + [(i, j)]
        if (i, j) == (Lx - 1, Ly - 1):
            out.append(acc)
            return
        for di, dj in STEPS:
            if i + di < Lx and j + dj < Ly:
                walk(i + di, j + dj, acc)
    walk(0, 0, [])
    return out


def brute_force_cost(d):
    return min(path_cost(d, p) for p in monotone_paths(*d.shape))


def path_metrics(path, f0_x, f0_y):
    """-> (pairs, pairs voiced in both, sum over those of (1200 log2(f0_x / f0_y))^2, pairs whose voicing differs)"""
    pairs = both = differ = 0
    sq = 0.0
    for i, j in path:
        fx, fy = float(f0_x[i]), float(f0_y[j])
        pairs += 1
        if fx > 0 and fy > 0:
            both += 1
            sq += (1200.0 * np.log2(fx / fy)) ** 2
        elif (fx > 0) != (fy > 0):
            differ += 1
    return pairs, both, sq, differ


def is_monotone_path(path, Lx, Ly):
    if not path or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (Lx - 1, Ly - 1):
        return False
    return all((c - a, d - b) in STEPS for (a, b), (c, d) in zip(path[:-1], path[1:]))

