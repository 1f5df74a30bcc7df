"""DiagGaussianMixture: sklearn.mixture.GaussianMixture(covariance_type='diag') fitted on the device (csrc/gmm_fit.hip).

The fit follows scikit-learn 1.7 step for step - KMeans(n_init=1) or k-means++ / random_from_data initialisation, then EM until
|change of the lower bound| < tol - in the dtype of X (float32 or float64).  Every random draw is taken on the host from
check_random_state(random_state) in scikit-learn's order (random_state=None: numpy's global generator, as the reference passes
none), so a seeded fit reproduces scikit-learn's.  The host reads back one or two scalars per Lloyd / EM iteration (the stop tests)
and nothing else.  There is no CPU fallback: the parameters live on the device, and score_samples / predict_proba / predict run there.
"""
import numpy as np
import torch

from .ops import _p, _stream, call, query

SUPPORTED_INIT = ('kmeans', 'k-means++', 'random_from_data')


def _rs(random_state):
    from sklearn.utils import check_random_state
    return check_random_state(random_state)


def _dev_x(X, device):
    if isinstance(X, torch.Tensor):
        x = X.detach()
        if x.dtype not in (torch.float32, torch.float64):
            x = x.double()
        x = x.to(device)
    else:
        a = np.asarray(X)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        x = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if x.dim() != 2:
        raise ValueError('X must be 2-D, got shape %s' % (tuple(x.shape),))
    return x.contiguous()


def kmeans_plusplus_draws(n, n_clusters, random_state, dtype=np.float64, n_local_trials=None):
    """The draws sklearn.cluster.kmeans_plusplus makes, in its order: (first center, uniforms [K-1, L])."""
    L = 2 + int(np.log(n_clusters)) if n_local_trials is None else n_local_trials
    w = np.ones(n, dtype=dtype)
    first = int(random_state.choice(n, p=w / w.sum()))
    u = np.stack([random_state.uniform(size=L) for _ in range(n_clusters - 1)]) if n_clusters > 1 else np.zeros((0, L))
    return first, u


def kmeans_plusplus(X, n_clusters, random_state=None, center=False, labels=None, n_local_trials=None):
    """Device k-means++ on X (minus its column mean with center=True, as KMeans.fit seeds) -> (centers [K, D] of the possibly
    centred X, indices int64 numpy [K]).  labels (device int32 [n], optional): labels[indices[c]] = c."""
    x = X
    n, D = x.shape
    db = x.element_size()
    rs = _rs(random_state)
    mean = column_mean(x) if center else None
    first, u = kmeans_plusplus_draws(n, n_clusters, rs, np.float32 if db == 4 else np.float64, n_local_trials)
    L = u.shape[1]
    dev = x.device
    ud = torch.from_numpy(np.ascontiguousarray(u, np.float64)).to(dev) if n_clusters > 1 else None
    idx = torch.empty(n_clusters, dtype=torch.int64, device=dev)
    centers = torch.empty(n_clusters, D, dtype=x.dtype, device=dev)
    nb = int(query("cpg_kmeans_pp_workspace", n, L))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    call("cpg_kmeans_pp", _p(x), n, D, db, _p(mean), first, _p(ud), n_clusters, L, _p(idx), _p(centers), _p(labels),
         _p(ws), nb, _stream())
    return centers, idx.cpu().numpy(), mean


def _colstats(x, shift=None):
    n, D = x.shape
    G = min(256, n)
    ws = torch.empty(G * 2 * D, dtype=torch.float64, device=x.device)
    out = torch.empty(2, D, dtype=torch.float64, device=x.device)
    call("cpg_gmm_colstats", _p(x), n, D, x.element_size(), _p(shift), _p(out), _p(ws), ws.numel() * 8, _stream())
    return out


def column_mean(x):
    """X.mean(axis=0) in the dtype of X (device)."""
    return (_colstats(x)[0] / x.shape[0]).to(x.dtype)


def kmeans_lloyd(x, centers, mean, tol, max_iter=300):
    """_kmeans_single_lloyd on x - mean from centers (of x - mean) -> (labels int32 [n], centers of x - mean, n_iter)."""
    n, D = x.shape
    K = centers.shape[0]
    db = x.element_size()
    dev = x.device
    nb = int(query("cpg_gmm_workspace", n, D, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rowdist = torch.empty(n, dtype=x.dtype, device=dev)
    status = torch.empty(2, dtype=torch.float64, device=dev)
    cur, nxt = centers.contiguous().clone(), torch.empty_like(centers)
    strict = False
    for i in range(max_iter):
        call("cpg_kmeans_lloyd_step", _p(x), n, D, K, db, _p(mean), _p(cur), _p(nxt), _p(labels), _p(rowdist), _p(status), 1,
             _p(ws), nb, _stream())
        cur, nxt = nxt, cur
        changed, shift = status.tolist()
        if changed == 0:
            strict = True
            break
        if shift <= tol:
            break
    if not strict:   # labels that match the returned centers
        call("cpg_kmeans_lloyd_step", _p(x), n, D, K, db, _p(mean), _p(cur), None, _p(labels), None, None, 0, None, 0, _stream())
    return labels, cur, i + 1


class DiagGaussianMixture:
    """sklearn.mixture.GaussianMixture(covariance_type='diag', n_init=1) on the device.  Fitted arrays are numpy arrays in the
    dtype of X (the attributes the reference and density_modeling read); the parameter block stays on the device for scoring."""
    covariance_type = 'diag'

    def __init__(self, n_components=1, *, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params='kmeans', weights_init=None, means_init=None, precisions_init=None, random_state=None,
                 warm_start=False, device=None, verbose=0, verbose_interval=10, timing=False):
        if covariance_type != 'diag':
            raise ValueError("DiagGaussianMixture fits covariance_type='diag' only, got %r" % (covariance_type,))
        if n_init != 1:
            raise ValueError('DiagGaussianMixture supports n_init=1 only, got %r' % (n_init,))
        if warm_start:
            raise ValueError('DiagGaussianMixture does not support warm_start')
        if init_params not in SUPPORTED_INIT:
            raise ValueError('init_params must be one of %s, got %r' % (SUPPORTED_INIT, init_params))
        self.n_components = int(n_components)
        if not 1 <= self.n_components <= 128:
            raise ValueError('n_components must be in [1, 128], got %d' % self.n_components)
        self.tol, self.reg_covar, self.max_iter = float(tol), float(reg_covar), int(max_iter)
        self.init_params = init_params
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.random_state = random_state
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.timing = timing   # record device events per phase: timings_ (ms) after fit (tools/gmm_fit_bench.py)

    def _mark(self, name):
        if self.timing:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((name, ev))

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def _block(self):
        return torch.empty(int(query("cpg_gmm_params_elems", self._D, self.n_components)), dtype=self._dtype, device=self.device)

    def _views(self, blk):
        K, D = self.n_components, self._D
        KD = K * D
        o = 4 * K
        return dict(w=blk[:K], means=blk[o:o + KD].view(K, D), covars=blk[o + KD:o + 2 * KD].view(K, D),
                    pchol=blk[o + 2 * KD:o + 3 * KD].view(K, D))

    def _init_labels(self, x, rs):
        n = x.shape[0]
        K = self.n_components
        if self.init_params == 'kmeans':
            # KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X): seeds on X - X.mean(0), tol = mean(var(X, 0)) * 1e-4
            centers, _, mean = kmeans_plusplus(x, K, rs, center=True)
            self._mark('seeding')
            var = _colstats(x, mean.double())[1] / n
            tol = float(var.mean()) * 1e-4
            labels, _, self._kmeans_n_iter = kmeans_lloyd(x, centers, mean, tol)
            self._mark('lloyd')
            return labels
        labels = torch.full((n,), -1, dtype=torch.int32, device=x.device)
        if self.init_params == 'k-means++':
            kmeans_plusplus(x, K, rs, center=False, labels=labels)
        else:   # random_from_data
            idx = rs.choice(n, size=K, replace=False)
            labels[torch.from_numpy(np.asarray(idx, np.int64)).to(x.device)] = torch.arange(K, dtype=torch.int32, device=x.device)
        return labels

    def fit(self, X, y=None):
        x = _dev_x(X, self.device)
        n, D = x.shape
        K = self.n_components
        if n < K:
            raise ValueError('Expected n_samples >= n_components but got n_components = %d, n_samples = %d' % (K, n))
        if D > 128:
            raise ValueError('DiagGaussianMixture takes at most 128 features, got %d' % D)
        self._dtype, self._D, self.n_features_in_ = x.dtype, D, D
        self._marks = []
        self._mark('start')
        db = x.element_size()
        nb = int(query("cpg_gmm_workspace", n, D, K))
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        cur, nxt = self._block(), self._block()
        npdt = np.float32 if db == 4 else np.float64
        have_all = self.weights_init is not None and self.means_init is not None and self.precisions_init is not None
        if not have_all:
            labels = self._init_labels(x, _rs(self.random_state))
            call("cpg_gmm_em_step", _p(x), n, D, K, db, None, _p(labels), self.reg_covar, _p(cur), None, _p(ws), nb, _stream())
        v = self._views(cur)
        if self.weights_init is not None:
            v['w'].copy_(torch.from_numpy(np.asarray(self.weights_init, npdt).reshape(K)))
        if self.means_init is not None:
            v['means'].copy_(torch.from_numpy(np.asarray(self.means_init, npdt).reshape(K, D)))
        if self.precisions_init is not None:
            v['pchol'].copy_(torch.from_numpy(np.sqrt(np.asarray(self.precisions_init, npdt).reshape(K, D))))
        call("cpg_gmm_params_prepare", _p(cur), D, K, db, _stream())
        self._mark('init')
        lbs = torch.empty(max(self.max_iter, 1), dtype=torch.float64, device=self.device)
        lower_bound, self.converged_, self.lower_bounds_ = -np.inf, False, []
        n_iter = 0
        for n_iter in range(1, self.max_iter + 1):
            prev = lower_bound
            call("cpg_gmm_em_step", _p(x), n, D, K, db, _p(cur), None, self.reg_covar, _p(nxt), _p(lbs[n_iter - 1:]), _p(ws), nb,
                 _stream())
            cur, nxt = nxt, cur
            self._mark('em')
            lower_bound = float(lbs[n_iter - 1].item())
            self.lower_bounds_.append(lower_bound)
            if abs(lower_bound - prev) < self.tol:
                self.converged_ = True
                break
        self._params = cur
        if self.timing:
            torch.cuda.synchronize()
            t = {'seeding': 0.0, 'lloyd': 0.0, 'init': 0.0, 'em': 0.0}
            passes = []
            for (_, a), (name, b) in zip(self._marks, self._marks[1:]):
                ms = a.elapsed_time(b)
                t[name] += ms
                if name == 'em':
                    passes.append(ms)
            t['em_iter_ms'] = passes
            self.timings_ = t
        self.n_iter_ = n_iter
        self.lower_bound_ = lower_bound
        v = self._views(cur)
        self.weights_ = v['w'].cpu().numpy().copy()
        self.means_ = v['means'].cpu().numpy().copy()
        self.precisions_cholesky_ = v['pchol'].cpu().numpy().copy()
        self.precisions_ = self.precisions_cholesky_ ** 2
        # covariances_: what the last M-step formed (or the initial ones, from precisions_init, if no EM iteration ran)
        self.covariances_ = v['covars'].cpu().numpy().copy() if (n_iter or not have_all) else 1.0 / self.precisions_
        return self

    # ---- scoring on the device -------------------------------------------------------------------------------------------
    def _score(self, X, lpn=False, resp=False, label=False):
        if not hasattr(self, '_params'):
            raise ValueError('This DiagGaussianMixture instance is not fitted yet: call fit first')
        x = _dev_x(X, self.device)
        if x.dtype != self._dtype:
            x = x.to(self._dtype)
        n, D = x.shape
        if D != self._D:
            raise ValueError('X has %d features, the mixture was fitted on %d' % (D, self._D))
        K = self.n_components
        o_l = torch.empty(n, dtype=x.dtype, device=x.device) if lpn else None
        o_r = torch.empty(n, K, dtype=x.dtype, device=x.device) if resp else None
        o_a = torch.empty(n, dtype=torch.int32, device=x.device) if label else None
        call("cpg_gmm_score", _p(x), n, D, K, x.element_size(), _p(self._params), _p(o_l), _p(o_r), _p(o_a), _stream())
        return o_l, o_r, o_a

    def score_samples(self, X):
        return self._score(X, lpn=True)[0].cpu().numpy()

    def score(self, X, y=None):
        return float(self.score_samples(X).mean())

    def predict_proba(self, X):
        return self._score(X, resp=True)[1].cpu().numpy()

    def predict(self, X):
        return self._score(X, label=True)[2].cpu().numpy().astype(np.int64)

