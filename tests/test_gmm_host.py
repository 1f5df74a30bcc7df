"""Host side of the device mixture fit (cpg/gmm.py): its random draws leave numpy's generator exactly where scikit-learn's
k-means++ leaves it, so a seeded device fit consumes the same stream as GaussianMixture.fit.  No GPU needed."""
import numpy as np
import pytest
from sklearn.cluster import kmeans_plusplus

from cpg.gmm import DiagGaussianMixture, kmeans_plusplus_draws


@pytest.mark.parametrize("n,K,D,dtype,seed", [(6000, 5, 14, np.float64, 0), (6000, 5, 14, np.float64, 1238),
                                              (2000, 100, 8, np.float32, 3), (500, 1, 4, np.float64, 7)])
def test_draw_schedule_leaves_global_state_where_kmeans_plusplus_does(n, K, D, dtype, seed):
    X = np.random.RandomState(seed + 100).randn(n, D).astype(dtype)
    np.random.seed(seed)
    _, idx = kmeans_plusplus(X, K)                 # random_state=None: numpy's global generator
    after_sklearn = np.random.get_state()
    np.random.seed(seed)
    first, u = kmeans_plusplus_draws(n, K, np.random.mtrand._rand, dtype)
    after_ours = np.random.get_state()
    assert first == idx[0]
    assert u.shape == (K - 1, 2 + int(np.log(K)))
    assert after_sklearn[0] == after_ours[0] and np.array_equal(after_sklearn[1], after_ours[1])
    assert after_sklearn[2:] == after_ours[2:]


@pytest.mark.parametrize("kw", [dict(covariance_type='full'), dict(covariance_type='tied'), dict(n_init=2),
                                dict(warm_start=True), dict(init_params='random'), dict(n_components=129)])
def test_unsupported_options_raise(kw):
    args = dict(n_components=3)
    args.update(kw)
    with pytest.raises(ValueError):
        DiagGaussianMixture(**args)


def test_density_modeling_rejects_unknown_fit_route():
    import torch
    from density_modeling import mogQ
    with pytest.raises(ValueError, match="fit must be"):
        mogQ(torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64), n_components=1, fit='cpu')
