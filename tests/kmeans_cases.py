"""The inputs of the k-means device tests (tests/test_kmeans_gpu.py), shared with the host test that shows they are clear
(tests/test_kmeans_cpu.py): Gaussian rows against Gaussian centroids at the shapes where the kernels change path, and a planted
clustering for Lloyd's loop. The row tile of the assign kernel is 64 rows, its LDS stage 32 centroids, KMEANS_SEGMENT 512 rows."""
import numpy as np

# (n, d, C): n around the 16-row wave tile and the 64-row workgroup tile, d at the ends, at the register form (64) and beside it,
# C around the 16-centroid MFMA tile, the 32-centroid stage and the maximum
ASSIGN_CASES = (
    (1, 4, 1), (15, 8, 2), (16, 64, 15), (17, 68, 16), (63, 252, 17), (64, 256, 31), (65, 64, 32), (65, 4, 33), (129, 64, 255),
    (1000, 64, 256), (1003, 256, 256), (200, 8, 256), (300, 252, 255), (1000, 68, 33), (64, 64, 1), (1, 256, 2),
)

# (n, d, C): n around KMEANS_SEGMENT, C at the slice widths of the update (64 / 32 / 16 columns), d at the ends
UPDATE_CASES = (
    (511, 4, 1), (512, 64, 16), (513, 256, 17), (1025, 64, 256), (513, 4, 256), (700, 256, 256), (1025, 68, 100),
)


def case_id(case):
    return "n%d-d%d-C%d" % case


def gaussian(n, d, C, seed=0):
    """(T float32 [n x d], Cen float32 [C x d])"""
    rng = np.random.default_rng([seed, n, d, C])
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((C, d)).astype(np.float32)


def random_assign(n, C, seed=0):
    """int32 [n] in [0, C), every cluster hit where n allows"""
    rng = np.random.default_rng([seed, n, C, 7])
    a = rng.integers(0, C, size=n).astype(np.int32)
    a[:min(n, C)] = rng.permutation(C)[:min(n, C)]
    return a


PLANTED = dict(d=64, sizes=(90, 40, 25, 70, 14, 33), noise=0.04, seed=3)


def planted(d=PLANTED["d"], sizes=PLANTED["sizes"], noise=PLANTED["noise"], seed=PLANTED["seed"]):
    """(T float32 [n x d] in shuffled row order, init int64 [C], truth int64 [n]): len(sizes) groups of unequal size around unit
    directions, the LAST group's direction a copy of the first one's (one planted direction duplicated), Gaussian noise of `noise`
    per component; init = the first row of every group."""
    rng = np.random.default_rng(seed)
    C = len(sizes)
    dirs = rng.standard_normal((C, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs[C - 1] = dirs[0]
    truth = np.repeat(np.arange(C), sizes)
    T = dirs[truth] * rng.uniform(0.5, 2.0, size=truth.size)[:, None] + noise * rng.standard_normal((truth.size, d))
    order = rng.permutation(truth.size)
    T, truth = T[order].astype(np.float32), truth[order]
    init = np.asarray([int(np.flatnonzero(truth == c)[0]) for c in range(C)], dtype=np.int64)
    return T, init, truth
