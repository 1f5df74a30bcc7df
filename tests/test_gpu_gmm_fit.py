"""Device fit of the CLaSS proposal Q(z) (cpg.gmm.DiagGaussianMixture, csrc/gmm_fit.hip) against scikit-learn and against the
reference's own fitted mixture (tests/golden/class_small.npz)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X: no CUDA/HIP device visible")


def _blobs(n, D, K, seed, dtype=np.float32, spread=4.0):
    rs = np.random.RandomState(seed)
    centers = rs.randn(K, D) * spread
    lab = rs.randint(0, K, size=n)
    X = centers[lab] + rs.randn(n, D) * rs.uniform(0.5, 1.5, size=(K, 1))[lab]
    return X.astype(dtype)


def _class_small_input():
    """tests/golden/make_golden.py::class_vectors up to the mixture fit: mu, logvar, then the seeds of the fit."""
    rng = np.random.RandomState(1238)
    N, D = 600, 14
    mu = torch.from_numpy(rng.randn(N, D) * 0.8)
    logvar = torch.from_numpy(rng.randn(N, D) * 0.1 - 2.0)
    torch.manual_seed(1238)
    np.random.seed(1238)
    return mu, logvar


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def test_mogQ_gpu_fit_pinned_to_reference(golden):
    from density_modeling import mogQ
    g = golden("class_small")
    mu, logvar = _class_small_input()
    Q = mogQ(mu, logvar, n_components=5, z_num_samples=10, covariance_type='diag', fit='gpu')
    assert Q.z.dtype == torch.float64 and Q.z.shape == (6000, 14)
    m = Q.mog
    assert m.n_iter_ == 10 and m.converged_
    assert m.means_.dtype == np.float64
    np.testing.assert_allclose(m.means_, g["gmm_means"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(m.covariances_, g["gmm_covars"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(m.weights_, g["gmm_weights"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(Q._c, g["gmm_covars"], rtol=1e-8)   # what the sampler uploaded


@pytest.mark.parametrize("n,D,K,dtype,seeds", [(6000, 14, 5, np.float64, (0, 1, 1238)),
                                               (200_000, 100, 100, np.float32, (0, 5))])
def test_kmeans_plusplus_indices(n, D, K, dtype, seeds):
    from sklearn.cluster import kmeans_plusplus as sk_kpp
    from cpg.gmm import kmeans_plusplus
    X = _blobs(n, D, K, 11, dtype) if dtype == np.float32 else np.random.RandomState(3).randn(n, D).astype(dtype)
    x = torch.from_numpy(X).cuda()
    Xc = X - X.mean(0)
    for s in seeds:
        _, want = sk_kpp(Xc, K, random_state=s)
        centers, got, _ = kmeans_plusplus(x, K, s, center=True)
        if dtype == np.float32 and not np.array_equal(got, want):
            _assert_same_seeding(Xc, got, want)
            continue
        np.testing.assert_array_equal(got, want)
        # the column mean is an f64 sum on the device, numpy's a pairwise f32 one: the centred rows agree to the mean's rounding
        np.testing.assert_allclose(centers.cpu().numpy(), (X - X.mean(0))[want], rtol=0, atol=1e-4)


def _assert_same_seeding(Xc, got, want):
    """float32: scikit-learn forms current_pot with a float32 BLAS product (relative error ~1e-6 at N = 2e5), and every
    u * current_pot target moves by that much - about a fifth of one row's weight - so candidate rows can differ from the step
    where a target lands that close to a row boundary.  The device keeps the potential exact to f64 and rounds it to float32 once.
    The sequences must agree from the start, and the seedings must be as good (potential of all K centers within 10 %)."""
    c = int(np.argmax(got != want))
    assert c >= 5, c
    X = Xc.astype(np.float64)

    def potential(idx):
        closest = np.full(X.shape[0], np.inf)
        for i in idx:
            closest = np.minimum(closest, ((X - X[i]) ** 2).sum(1))
        return closest.sum()
    pg, pw = potential(got), potential(want)
    assert abs(pg - pw) <= 0.10 * pw, (c, pg, pw)


def test_lloyd_against_sklearn_kmeans():
    from sklearn.cluster import KMeans, kmeans_plusplus as sk_kpp
    from cpg.gmm import column_mean, kmeans_lloyd
    n, D, K = 200_000, 100, 100
    X = _blobs(n, D, K, 21, spread=1.0)   # overlapping enough that Lloyd takes several iterations
    Xc = X - X.mean(0)
    init, _ = sk_kpp(Xc, K, random_state=4)
    km = KMeans(K, init=init + X.mean(0), n_init=1).fit(X)
    x = torch.from_numpy(X).cuda()
    mean = column_mean(x)
    tol = float(np.mean(np.var(X, axis=0))) * 1e-4
    labels, centers, n_iter = kmeans_lloyd(x, torch.from_numpy(init).cuda(), mean, tol)
    assert n_iter == km.n_iter_
    np.testing.assert_array_equal(labels.cpu().numpy(), km.labels_)
    c = centers.cpu().numpy() + X.mean(0)
    np.testing.assert_allclose(c, km.cluster_centers_, rtol=1e-5, atol=1e-5 * np.abs(km.cluster_centers_).max())


def _params_close(m, ref, ref64=None, cov_rtol=1e-4):
    """means within 1e-4 absolute, covariances and weights within 1e-4 relative, of scikit-learn in float64 on the same data
    (or within twice scikit-learn's own float32 error there, if that is larger).  scikit-learn's float32 covariance is
    avg_X2 - 2 avg_X_means + avg_means2 with float32 sums over every row: where means^2 >> var it loses ~1e-3 to cancellation,
    while the device sums in f64.  Without a float64 run, cov_rtol bounds the float32 disagreement directly."""
    if ref64 is None:
        np.testing.assert_allclose(m.means_, ref.means_, rtol=0, atol=1e-4)
        assert _rel(m.covariances_, ref.covariances_) < cov_rtol
        assert _rel(m.weights_, ref.weights_) < 1e-4
        return
    bar = max(1e-4, 2 * float(np.max(np.abs(ref.means_ - ref64.means_))))
    assert float(np.max(np.abs(m.means_ - ref64.means_))) < bar
    for a in ('covariances_', 'weights_'):
        bar = max(1e-4, 2 * _rel(getattr(ref, a), getattr(ref64, a)))
        assert _rel(getattr(m, a), getattr(ref64, a)) < bar, (a, _rel(getattr(m, a), getattr(ref64, a)), bar)


def test_em_from_explicit_parameters():
    from sklearn.mixture import GaussianMixture
    from cpg.gmm import DiagGaussianMixture
    n, D, K = 200_000, 100, 100
    X = _blobs(n, D, K, 31, spread=1.5)
    rs = np.random.RandomState(9)
    # float32 initial parameters: float64 ones would make scikit-learn run the whole EM in float64 (10 eps(float64) in nk)
    w = np.r_[np.full(72, 1 / 128), np.full(28, 1 / 64)].astype(np.float32)   # sums to 1 exactly in float32
    init = dict(weights_init=w, means_init=X[rs.choice(n, K, replace=False)],
                precisions_init=np.full((K, D), 0.5, np.float32))
    kw = dict(n_components=K, covariance_type='diag', max_iter=5, tol=0, **init)
    ref = GaussianMixture(**kw).fit(X)
    kw64 = dict(kw, **{k: np.asarray(v, np.float64) for k, v in init.items()})
    ref64 = GaussianMixture(**kw64).fit(X.astype(np.float64))
    m = DiagGaussianMixture(**kw).fit(torch.from_numpy(X).cuda())
    assert m.n_iter_ == ref.n_iter_ == 5 and m.converged_ == ref.converged_
    _params_close(m, ref, ref64)
    assert len(m.lower_bounds_) == len(ref.lower_bounds_) == 5
    for a, b in zip(m.lower_bounds_, ref.lower_bounds_):
        assert abs(a - b) <= 1e-5 * abs(b), (m.lower_bounds_, ref.lower_bounds_)
    np.testing.assert_allclose(m.precisions_cholesky_ ** 2, m.precisions_, rtol=1e-6)


@pytest.fixture(scope="module")
def default_fit():
    from sklearn.mixture import GaussianMixture
    from cpg.gmm import DiagGaussianMixture
    X = _blobs(200_000, 100, 100, 41)
    ref = GaussianMixture(n_components=100, covariance_type='diag', random_state=0).fit(X)
    m = DiagGaussianMixture(n_components=100, covariance_type='diag', random_state=0).fit(torch.from_numpy(X).cuda())
    return X, ref, m


def test_full_default_fit(default_fit):
    X, ref, m = default_fit
    lbs = ref.lower_bounds_
    last = abs(lbs[-1] - lbs[-2]) if len(lbs) > 1 else abs(lbs[-1])
    assert last <= ref.tol / 2 or last >= 2 * ref.tol, "scikit-learn's last change sits too close to tol for a fair comparison"
    assert m.n_iter_ == ref.n_iter_ and m.converged_ == ref.converged_
    _params_close(m, ref, cov_rtol=2e-3)
    assert abs(m.lower_bound_ - ref.lower_bound_) <= 1e-5 * abs(ref.lower_bound_)


def test_score_predict_against_sklearn(default_fit):
    X, ref, m = default_fit
    Xs = X[:20_000]
    sk = type(ref)(n_components=m.n_components, covariance_type='diag')   # scikit-learn carrying the device fit's parameters
    sk.weights_, sk.means_, sk.covariances_ = m.weights_, m.means_, m.covariances_
    sk.precisions_cholesky_, sk.precisions_ = m.precisions_cholesky_, m.precisions_
    want = sk.score_samples(Xs)
    got = m.score_samples(Xs)
    # both evaluate sum means^2 prec - 2 X.(means prec)^T + X^2 prec^T in float32: terms of ~1e3 cancel to ~1e2, so the two orders
    # of summation differ by a few float32 ulps of the terms
    assert _rel(got, want) < 5e-5
    assert abs(m.score(Xs) - sk.score(Xs)) <= 1e-5 * abs(sk.score(Xs))
    pp, spp = m.predict_proba(Xs), sk.predict_proba(Xs)
    np.testing.assert_allclose(pp, spp, rtol=1e-5, atol=2e-4)   # scikit-learn's float32 log-densities carry ~1e-4 absolute
    assert np.mean(m.predict(Xs) == sk.predict(Xs)) > 0.999


def test_mogQ_gpu_then_rejection_sample_and_errors():
    import types
    from density_modeling import mogQ
    mu, logvar = _class_small_input()
    Q = mogQ(mu, logvar, n_components=5, z_num_samples=10, covariance_type='diag', fit='gpu')
    clf = types.SimpleNamespace(coef_=np.ones((1, 14)) * 0.1, intercept_=np.array([0.0]), classes_=np.array([0.0, 1.0]))
    Q.init_attr_classifiers({'amp': clf}, clf_targets={'amp': 1})
    z, scores, acc = Q.rejection_sample(512)
    assert z.shape == (512, 14) and torch.isfinite(z).all() and acc.dtype == bool
    assert np.isfinite(Q.logpdf(z[0].double()))
    with pytest.raises(ValueError):
        mogQ(mu, logvar, n_components=5, covariance_type='full', fit='gpu')


def test_sample_pipeline_with_gpu_fit(tmp_path, monkeypatch):
    import importlib
    import cfg
    importlib.reload(cfg)
    import tb_json_logger
    import losses
    tb_json_logger.reset()
    losses.rf.clear()
    monkeypatch.chdir(tmp_path)
    import main
    import sample_pipeline as sp
    common = ['--tiny', '1', '--phase', '1', '--runname', 'gmmfit', '--hw.synthetic_size', '2048']
    try:
        main.run(common)
        importlib.reload(cfg)
        samples = sp.run(common + ['--Q_fit', 'gpu', '--Q_n_components', '8', '--n_samples_per_round', '512',
                                   '--n_samples_acc', '10', '--samples_outfn_prefix', 'smp'])
        assert samples['accept'].sum() >= 10
    finally:
        importlib.reload(cfg)
        tb_json_logger.reset()
        losses.rf.clear()
        losses.set_prior_sampler(None)


def test_reference_size_em_properties():
    from cpg.gmm import DiagGaussianMixture
    n, D, K = 1_000_000, 100, 100
    rs = np.random.RandomState(51)
    X = (rs.randn(n, D) * 0.7 + 0.3 * rs.randn(1, D)).astype(np.float32)   # one overlapping blob, like a WAE latent
    m = DiagGaussianMixture(n_components=K, random_state=0, max_iter=20).fit(torch.from_numpy(X).cuda())
    for a in (m.weights_, m.means_, m.covariances_, m.precisions_cholesky_):
        assert np.isfinite(a).all()
    assert abs(float(np.sum(m.weights_, dtype=np.float64)) - 1.0) < 1e-5
    lb = np.asarray(m.lower_bounds_)
    assert np.all(np.diff(lb) >= -1e-6 * np.abs(lb[1:])), lb
