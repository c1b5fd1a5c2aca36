"""Host side of the BGMM fit (include/ppk.h, section "BGMM fit").

  * `findWithinLabel` / `findBetweenLabel_bgmm` : PopPUNK/bgmm.py:48-97 on the fitted means and the assigned labels
  * `seeding_positions` / `kmeanspp_centres`   : the seeded draw of the own initialisation's starting centres.  This is
                                                  the project's definition, standing where sklearn draws k-means from
                                                  numpy's global random state (which cannot be reproduced): run r uses
                                                  `numpy.random.default_rng(seed + r)`
  * `FitResult`                                 : a `ppk_bgmm_fit_result` as numpy arrays
The arithmetic of the fit itself is in libppk_hip.so (csrc/ppk_bgmm_fit.hip): the passes over the rows on the device,
the M-step and the lower bound in double on the host.
"""
import numpy as np

SEED_SAMPLE = 4096          # rows the k-means++ draw looks at


def within_from_counts(means, counts, rank=0):
    """findWithinLabel from the number of rows per label."""
    means = np.asarray(means, dtype=np.float64)
    used = [(k, float(np.linalg.norm(means[k]))) for k in range(means.shape[0]) if counts[k] > 0]
    return sorted(used, key=lambda t: t[1])[rank][0]


def between_from_counts(counts):
    """findBetweenLabel_bgmm from the number of rows per label."""
    return int(np.argmax(np.asarray(counts)))


def findWithinLabel(means, assignments, rank=0):
    """PopPUNK/bgmm.py:71-97: the used component whose mean is nearest the origin (the first on ties: a stable sort
    on the norm)."""
    K = np.asarray(means).shape[0]
    return within_from_counts(means, np.bincount(np.asarray(assignments).astype(np.int64), minlength=K)[:K], rank)


def findBetweenLabel_bgmm(means, assignments):
    """PopPUNK/bgmm.py:48-69: the component with most rows assigned to it (the first on ties)."""
    K = np.asarray(means).shape[0]
    return between_from_counts(np.bincount(np.asarray(assignments).astype(np.int64), minlength=K)[:K])


def seeding_positions(n_train, rng):
    """Positions (in training order) of the rows the draw looks at: all of them up to SEED_SAMPLE rows, otherwise
    SEED_SAMPLE positions drawn with replacement.  None: every row."""
    if n_train <= SEED_SAMPLE:
        return None
    return rng.integers(0, n_train, size=SEED_SAMPLE)


def kmeanspp_centres(points, K, rng):
    """k-means++ on `points` (float64 [m, 2], scaled training rows): the first centre uniformly, each further one with
    probability proportional to the squared distance to the nearest centre so far (uniformly when every distance is
    0: fewer distinct points than centres)."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    m = P.shape[0]
    centres = np.empty((K, 2), dtype=np.float64)
    centres[0] = P[int(rng.integers(m))]
    dx, dy = P[:, 0] - centres[0, 0], P[:, 1] - centres[0, 1]
    d2 = dx * dx + dy * dy
    for k in range(1, K):
        cum = np.cumsum(d2)
        if cum[-1] > 0.0:
            j = min(int(np.searchsorted(cum, rng.random() * cum[-1], side="right")), m - 1)
        else:
            j = int(rng.integers(m))
        centres[k] = P[j]
        dx, dy = P[:, 0] - centres[k, 0], P[:, 1] - centres[k, 1]
        d2 = np.minimum(d2, dx * dx + dy * dy)
    return centres


def initial_centres(fetch_rows, n_train, scale, K, seed, n_init):
    """float64 [n_init, K, 2]: the starting centres of runs 0 .. n_init - 1.  fetch_rows(positions or None) returns the
    un-scaled float32 rows at those training positions."""
    scale = np.asarray(scale, dtype=np.float32).reshape(2)
    out = np.empty((n_init, K, 2), dtype=np.float64)
    for r in range(n_init):
        rng = np.random.default_rng(int(seed) + r)
        rows = np.asarray(fetch_rows(seeding_positions(n_train, rng)), dtype=np.float32)
        out[r] = kmeanspp_centres((rows / scale).astype(np.float64), K, rng)
    return out


def state_arrays(state):
    """A `_lib.BgmmState` as a dict of numpy arrays trimmed to its K components."""
    K = state.K
    a = lambda f: np.ctypeslib.as_array(getattr(state, f)).copy()[:K]      # noqa: E731
    return {"weights": a("weights"), "means": a("means"), "covariances": a("covariances").reshape(K, 2, 2),
            "weight_concentration": np.stack([a("weight_conc_a"), a("weight_conc_b")]),
            "mean_precision": a("mean_precision"), "degrees_of_freedom": a("dof"), "chol": a("chol"),
            "lin": a("lin"), "log_const": a("log_const")}


class FitResult:
    """What a fit returns: the parameters of the best run (`weights`, `means`, `covariances`, `weight_concentration`
    [2, K], `mean_precision`, `degrees_of_freedom`), `n_iter`, `converged`, `lower_bound`, `lower_bounds` (one per
    iteration of the best run), `best_init`, `n_train`, `cov_prior`, and per run `init_lower_bounds`, `init_n_iter`,
    `kmeans_iter`.  `state` is the `_lib.BgmmState` itself."""

    def __init__(self, res):
        from . import _lib
        self.state = _lib.BgmmState.from_buffer_copy(res.state)
        for k, v in state_arrays(self.state).items():
            setattr(self, k, v)
        self.n_iter, self.converged = int(res.n_iter), bool(res.converged)
        self.best_init, runs = int(res.best_init), int(res.n_init_run)
        self.n_train = int(res.n_train)
        self.lower_bound = float(res.lower_bound)
        self.lower_bounds = np.ctypeslib.as_array(res.lower_bounds).copy()[:self.n_iter]
        self.cov_prior = np.ctypeslib.as_array(res.cov_prior).copy().reshape(2, 2)
        self.train_mean = np.ctypeslib.as_array(res.train_mean).copy()
        self.init_lower_bounds = np.ctypeslib.as_array(res.init_lower_bound).copy()[:runs]
        self.init_n_iter = np.ctypeslib.as_array(res.init_n_iter).copy()[:runs]
        self.kmeans_iter = np.ctypeslib.as_array(res.kmeans_iter).copy()[:runs]
