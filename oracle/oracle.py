"""CPU ORACLE — test infrastructure only, never shipped, never on the product path.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this module, and only as the *checker*.

A float64 NumPy restatement of the upstream algorithms the reference reaches at its three
hot-path call sites:

* ``IDF(2).fit(tf).idf`` + the 1e-4 floor ............ LDAClustering.scala:177-188
* ``lda.run(corpus)`` with ``OnlineLDAOptimizer`` ...... LDAClustering.scala:37-61 (switch :40-46)
* ``toLocal.topicDistribution(tf)`` ................... LDALoader.scala:108

The arithmetic lives in the third-party dependency ``org.apache.spark:spark-mllib_2.12:2.4.3``
(TextClustering/build.sbt:10) and Breeze 0.13.2; neither is present in this container (no
JVM, no jars).  Each function below names the upstream symbol it restates ([U] = upstream,
described from its published source, no line numbers available here).

Pinning: IDF is pinned bit-exactly by the reference's saved TF·IDF edges
(tests/golden/{en,ge}_idf.npz); ``describe_topics`` by the printed top terms; the E-step /
``dirichlet_expectation`` / ``digamma`` / ``topic_distribution`` by the 51×5 topic
proportions of Result_EN_*.  **Parity unpinned** (no in-reference artefact): the online
M-step trajectory (``update_lambda``/``update_alpha``), ``log_likelihood_bound``, and
HashingTF's murmur3 (pinned only by public MurmurHash3_x86_32 known answers for the
standard variant; the Spark-2.4 legacy tail variant is unpinned).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
from scipy.special import gammaln

# ---------------------------------------------------------------------------------------
# MurmurHash3_x86_32 + HashingTF   [U] mllib.feature.HashingTF.murmur3Hash / transform,
# spark-unsafe Murmur3_x86_32.hashUnsafeBytes (2.4.3: legacy per-byte tail) and
# hashUnsafeBytes2 (3.x: standard tail); Utils.nonNegativeMod.
# Reference slot: LDAClustering.scala:154-167 (vocab-indexed counting HashingTF replaces).
# ---------------------------------------------------------------------------------------
_C1, _C2 = 0xCC9E2D51, 0x1B873593
_M32 = 0xFFFFFFFF
HASH_STANDARD, HASH_SPARK24 = 0, 1


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M32


def _mix_k1(k1):
    k1 = (k1 * _C1) & _M32
    k1 = _rotl(k1, 15)
    return (k1 * _C2) & _M32


def _mix_h1(h1, k1):
    h1 ^= k1
    h1 = _rotl(h1, 13)
    return (h1 * 5 + 0xE6546B64) & _M32


def _fmix(h1, length):
    h1 ^= length & _M32
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & _M32
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & _M32
    h1 ^= h1 >> 16
    return h1


def murmur3_x86_32(data: bytes, seed: int = 42, variant: int = HASH_STANDARD) -> int:
    """Signed 32-bit MurmurHash3_x86_32 of ``data``.

    variant HASH_STANDARD: the published algorithm (= Spark 3.x ``hashUnsafeBytes2``).
    variant HASH_SPARK24: Spark 2.4.x ``hashUnsafeBytes`` — each of the len%4 tail bytes is
    sign-extended and mixed as its own 4-byte block (mixK1 + mixH1).
    """
    h1 = seed & _M32
    n = len(data)
    nb = n - (n % 4)
    for i in range(0, nb, 4):
        k1 = data[i] | (data[i + 1] << 8) | (data[i + 2] << 16) | (data[i + 3] << 24)
        h1 = _mix_h1(h1, _mix_k1(k1))
    if variant == HASH_SPARK24:
        for i in range(nb, n):
            b = data[i]
            if b >= 128:
                b -= 256
            h1 = _mix_h1(h1, _mix_k1(b & _M32))
    else:
        k1 = 0
        tail = n - nb
        if tail >= 3:
            k1 ^= data[nb + 2] << 16
        if tail >= 2:
            k1 ^= data[nb + 1] << 8
        if tail >= 1:
            k1 ^= data[nb]
            h1 ^= _mix_k1(k1)
    h = _fmix(h1, n)
    return h - (1 << 32) if h >= (1 << 31) else h


def non_negative_mod(x: int, mod: int) -> int:
    """[U] org.apache.spark.util.Utils.nonNegativeMod (Java ``%`` truncates toward 0)."""
    raw = int(math.fmod(x, mod))
    return raw + (mod if raw < 0 else 0)


# [U] ml.feature.Tokenizer.createTransformFunc: text.toLowerCase.split("\\s") — the step in front of
# HashingTF.  Java's \s (no UNICODE_CHARACTER_CLASS) is [ \t\n\x0B\f\r];
# String.split(regex) = split(regex, 0): interior empty strings kept, trailing ones removed, and a
# string with no match comes back whole ("" → [""]).
_JAVA_SPACE = " \t\n\x0b\f\r"


def java_split_whitespace(s: str):
    """Java ``s.split("\\s")`` (limit 0), restated with explicit loops."""
    pieces, cur, matched = [], [], False
    for ch in s:
        if ch in _JAVA_SPACE:
            pieces.append("".join(cur))
            cur, matched = [], True
        else:
            cur.append(ch)
    if not matched:
        return [s]
    pieces.append("".join(cur))
    while pieces and pieces[-1] == "":
        pieces.pop()
    return pieces


# Spark 2.4.3 runs on Java 8 (Unicode 6.2): code points assigned later are unassigned there and
# toLowerCase leaves them alone; Python's newer database (3.10: Unicode 13.0) lower-cases the cased
# additions of Unicode 7.0–13.0 (U+037F, U+0528–U+052F, U+A698–U+A69F, U+A794–U+A79F, U+A7AB–U+A7FF,
# Georgian Mtavruli U+1C90–U+1CBF; supplementary: Warang Citi, Old Hungarian, Osage, Medefaidrin,
# Adlam) and the Cherokee letters U+13A0–U+13FF, caseless in 6.2.  Case pairs are otherwise stable
# across Unicode versions, and String.toLowerCase(Locale.ROOT)'s special casings (U+0130 → "i̇",
# Final_Sigma for U+03A3) are Python's str.lower too.  (tools/gen_case_table.py holds the same BMP set.)
_JAVA8_IDENTITY_RANGES = ((0x37F, 0x37F), (0x528, 0x52F), (0x13A0, 0x13FF), (0x1C90, 0x1CBF), (0xA698, 0xA69F),
                          (0xA794, 0xA79F), (0xA7AB, 0xA7FF), (0x104B0, 0x104FF), (0x10C80, 0x10CFF),
                          (0x118A0, 0x118FF), (0x16E40, 0x16E9F), (0x1E900, 0x1E95F))


def java8_identity(cp: int) -> bool:
    return any(lo <= cp <= hi for lo, hi in _JAVA8_IDENTITY_RANGES)


def java_lower(text: str) -> str:
    """[U] java.lang.String.toLowerCase(Locale.ROOT) on Java 8, restated with str.lower."""
    if not any(java8_identity(ord(ch)) for ch in text if ord(ch) >= 0x37F):
        return text.lower()
    out, seg = [], []
    for ch in text:
        if java8_identity(ord(ch)):
            out.append("".join(seg).lower())
            out.append(ch)
            seg = []
        else:
            seg.append(ch)
    out.append("".join(seg).lower())
    return "".join(out)


def tokenize(text: str):
    """[U] Tokenizer: ``text.toLowerCase.split("\\s")`` (Java 8 lower-casing, Java split)."""
    return java_split_whitespace(java_lower(text))


def hashing_tf(docs, num_features=1 << 18, binary=False, variant=HASH_STANDARD):
    """[U] HashingTF.transform for each doc (a sequence of str tokens) → CSR (sorted indices).

    Returns (indptr int64[D+1], indices int32[nnz], values float64[nnz]).
    """
    indptr = [0]
    idx_all, val_all = [], []
    for toks in docs:
        tf = {}
        for t in toks:
            b = t.encode("utf-8") if isinstance(t, str) else bytes(t)
            i = non_negative_mod(murmur3_x86_32(b, 42, variant), num_features)
            tf[i] = 1.0 if binary else tf.get(i, 0.0) + 1.0
        ks = sorted(tf)
        idx_all.extend(ks)
        val_all.extend(tf[i] for i in ks)
        indptr.append(len(idx_all))
    return (np.asarray(indptr, np.int64), np.asarray(idx_all, np.int32),
            np.asarray(val_all, np.float64))


# ---------------------------------------------------------------------------------------
# IDF   [U] mllib.feature.IDF.fit (DocumentFrequencyAggregator.add/merge/idf), IDFModel.transform
# Reference: LDAClustering.scala:177 (new IDF(2).fit(tf).idf) and :180-192 (× idf, 0 → 1e-4).
# ---------------------------------------------------------------------------------------
def idf_fit(indptr, indices, values, num_features, min_doc_freq=0):
    """df_j = #docs with value_j > 0; m = #docs; idf_j = df_j >= minDocFreq ? ln((m+1)/(df_j+1)) : 0."""
    indices = np.asarray(indices)
    values = np.asarray(values)
    df = np.bincount(indices[values > 0], minlength=num_features).astype(np.int64)
    m = int(len(indptr) - 1)
    idf = np.where(df >= min_doc_freq, np.log((m + 1.0) / (df + 1.0)), 0.0)
    return idf, df, m


def idf_transform(indices, values, idf, floor=0.0):
    """IDFModel.transform on CSR values; ``floor`` > 0 reproduces LDAClustering.scala:184-187."""
    w = np.asarray(idf)[np.asarray(indices)]
    if floor:
        w = np.where(w == 0.0, floor, w)
    return np.asarray(values, np.float64) * w


# ---------------------------------------------------------------------------------------
# Breeze 0.13.2 special functions   [U] breeze.numerics.digamma / trigamma
# ---------------------------------------------------------------------------------------
def digamma(x):
    """Breeze digamma: recurrence up to x > 5, then the asymptotic series (vectorised)."""
    x = np.array(x, np.float64, copy=True)
    r = np.zeros_like(x)
    m = x <= 5
    while m.any():
        r[m] -= 1.0 / x[m]
        x[m] += 1.0
        m = x <= 5
    f = 1.0 / (x * x)
    t = f * (-1 / 12.0 + f * (1 / 120.0 + f * (-1 / 252.0 + f * (1 / 240.0 + f * (
        -1 / 132.0 + f * (691 / 32760.0 + f * (-1 / 12.0 + f * 3617 / 8160.0)))))))
    return r + np.log(x) - 0.5 / x + t


def trigamma(x):
    """Breeze trigamma: recurrence up to x > 5, then the asymptotic series (vectorised)."""
    x = np.array(x, np.float64, copy=True)
    r = np.zeros_like(x)
    m = x <= 5
    while m.any():
        r[m] += 1.0 / (x[m] * x[m])
        x[m] += 1.0
        m = x <= 5
    f = 1.0 / (x * x)
    t = f * (1 / 6.0 + f * (-1 / 30.0 + f * (1 / 42.0 + f * (-1 / 30.0 + f * (5 / 66.0 + f * (
        -691 / 2730.0 + f * (7 / 6.0 - f * 3617 / 510.0)))))))
    return r + 1.0 / x + f / 2.0 + t / x


# ---------------------------------------------------------------------------------------
# LDAUtils   [U] mllib.clustering.LDAUtils.dirichletExpectation / logSumExp
# ---------------------------------------------------------------------------------------
def dirichlet_expectation(a):
    """Vector: ψ(a) − ψ(Σa).  Matrix: row-wise ψ(A) − ψ(rowsum(A))[:, None]."""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        return digamma(a) - digamma(np.array([a.sum()]))[0]
    return digamma(a) - digamma(a.sum(axis=1))[:, None]


def log_sum_exp(x):
    a = np.max(x)
    return a + np.log(np.sum(np.exp(x - a)))


# ---------------------------------------------------------------------------------------
# Counter-based Gamma(shape, 1/shape) sampler shared with the HIP library (stc_rng.h).
# Spark draws γ₀ from java.util.Random → MersenneTwister → Breeze Gamma, which cannot be
# replayed here (SURVEY.md §7 hard part 7); this is the build's documented replacement.
# ---------------------------------------------------------------------------------------
_U64 = (1 << 64) - 1


def splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def _uniform(stream: int, ctr: int) -> float:
    x = splitmix64((stream + ctr * 0xD1B54A32D192ED03) & _U64)
    return ((x >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def doc_stream(seed: int, key: int) -> int:
    return splitmix64((seed & _U64) ^ splitmix64(key & _U64))


def gamma_sample(stream: int, topic: int, shape: float) -> float:
    """Marsaglia–Tsang Gamma(shape, 1/shape), 3 uniforms per attempt (Box–Muller normal)."""
    d = shape - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    v = 1.0
    for attempt in range(64):
        base = (topic << 8) + 3 * attempt
        u1 = _uniform(stream, base)
        u2 = _uniform(stream, base + 1)
        x = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        u = _uniform(stream, base + 2)
        if u < 1.0 - 0.0331 * (x * x) * (x * x):
            break
        if math.log(u) < 0.5 * x * x + d * (1.0 - v + math.log(v)):
            break
    return d * v / shape


def gamma_init(seed: int, key: int, k: int, shape: float = 100.0) -> np.ndarray:
    s = doc_stream(seed, key)
    return np.array([gamma_sample(s, t, shape) for t in range(k)], np.float64)


def train_doc_key(iteration: int, rank: int, batch_pos: int) -> int:
    """γ₀ key of the batch_pos-th member of minibatch ``iteration`` on ``rank`` (see stc.h)."""
    return ((iteration & 0xFFFFFF) << 40) | ((rank & 0xFF) << 32) | (batch_pos & 0xFFFFFFFF)


def init_lambda(seed: int, V: int, k: int, shape: float = 100.0) -> np.ndarray:
    """[U] OnlineLDAOptimizer.initialize: λ₀ ~ Gamma(shape, 1/shape) i.i.d. (Spark: k×V from its
    MT generator).  The counter-RNG replacement keyed by the k×V element index t·V + v, as
    stc_lda_init_random draws it.  Returned V×k (topicsMatrix orientation)."""
    lam = np.empty((V, k), np.float64)
    for t in range(k):
        for v in range(V):
            lam[v, t] = gamma_sample(doc_stream(seed, t * V + v), 0, shape)
    return lam


def sample_members(seed: int, draw: int, rank: int, n_docs: int, fraction: float,
                   with_replacement: bool) -> list:
    """[U] OnlineLDAOptimizer.next: ``docs.sample(withReplacement, miniBatchFraction, rng.nextLong())``
    — per document a Poisson(f) multiplicity (with replacement) or a Bernoulli(f) flag, from the
    counter RNG keyed (seed ^ 0x5DEECE66D, draw, rank, doc) as stc_lda_next draws it.  Returns the
    members in document order, a document repeated by its multiplicity (RDD.sample's order)."""
    out = []
    for d in range(n_docs):
        u = _uniform(doc_stream(seed ^ 0x5DEECE66D, train_doc_key(draw, rank, d)), 0)
        c = 0
        if with_replacement:  # Poisson by inversion (capped at 64 like the device)
            p = math.exp(-fraction)
            F = p
            while u > F and c < 64:
                c += 1
                p *= fraction / c
                F += p
        else:
            c = 1 if u < fraction else 0
        out.extend([d] * c)
    return out


# ---------------------------------------------------------------------------------------
# OnlineLDAOptimizer   [U] mllib.clustering.OnlineLDAOptimizer
# ---------------------------------------------------------------------------------------
def variational_topic_inference(ids, cts, exp_elog_beta, alpha, gamma0, max_iter=None, n_iter=None):
    """[U] OnlineLDAOptimizer.variationalTopicInference (the E-step fixed point).

    exp_elog_beta is V×k.  Returns (gamma[k], sstats[k, nnz], n_iter).  The loop has no cap
    upstream; ``max_iter`` exists only so a test can bound a pathological case, and ``n_iter`` runs
    exactly that many iterations (ignoring the stop rule) so a test can compare a run that stopped
    an iteration earlier or later than the oracle's at the same iteration.
    """
    cts = np.asarray(cts, np.float64)
    alpha = np.asarray(alpha, np.float64)
    k = alpha.size
    gamma = np.array(gamma0, np.float64, copy=True)
    e_theta = np.exp(dirichlet_expectation(gamma))
    B = exp_elog_beta[np.asarray(ids)]                       # nnz × k
    phi_norm = B @ e_theta + 1e-100
    mean_change = 1.0
    it = 0
    while (mean_change > 1e-3) if n_iter is None else (it < n_iter):
        last = gamma.copy()
        gamma = e_theta * (B.T @ (cts / phi_norm)) + alpha
        e_theta = np.exp(dirichlet_expectation(gamma))
        phi_norm = B @ e_theta + 1e-100
        mean_change = np.sum(np.abs(gamma - last)) / k
        it += 1
        if max_iter is not None and it >= max_iter:
            break
    sstats = np.outer(e_theta, cts / phi_norm)
    return gamma, sstats, it


@dataclass
class OnlineLDAState:
    """[U] OnlineLDAOptimizer fields: λ (k×V), α, η, iteration, τ0, κ, corpusSize, fraction."""
    lam: np.ndarray                    # k × V (Spark's internal orientation)
    alpha: np.ndarray
    eta: float
    corpus_size: int
    mini_batch_fraction: float = 0.05
    tau0: float = 1024.0
    kappa: float = 0.51
    optimize_doc_concentration: bool = False
    gamma_shape: float = 100.0
    iteration: int = 0
    history: list = field(default_factory=list)

    def rho(self):
        """[U] OnlineLDAOptimizer.rho: (τ0 + iteration)^(−κ)."""
        return math.pow(self.tau0 + self.iteration, -self.kappa)


def resolve_alpha_eta(k, doc_concentration=-1.0, topic_concentration=-1.0):
    """[U] OnlineLDAOptimizer.initialize: −1 ⇒ 1/k for α (per topic) and η."""
    dc = np.atleast_1d(np.asarray(doc_concentration, np.float64))
    if dc.size == 1:
        alpha = np.full(k, 1.0 / k) if dc[0] == -1 else np.full(k, dc[0])
    else:
        assert dc.size == k
        alpha = dc.copy()
    eta = 1.0 / k if topic_concentration == -1 else float(topic_concentration)
    return alpha, eta


def submit_minibatch(state: OnlineLDAState, docs, gamma0s):
    """[U] OnlineLDAOptimizer.submitMiniBatch + updateLambda + updateAlpha (one ``next()``).

    docs: list of (ids, cts); gamma0s: per-doc initial γ (k).  Returns diagnostics.
    """
    state.iteration += 1
    k, V = state.lam.shape
    exp_elog_beta = np.exp(dirichlet_expectation(state.lam)).T      # V × k
    stat = np.zeros((k, V))
    logphat = np.zeros(k)
    n_nonempty = 0
    iters = []
    for (ids, cts), g0 in zip(docs, gamma0s):
        if len(ids) == 0 or not np.any(np.asarray(cts) != 0):
            continue
        n_nonempty += 1
        gamma, sstats, it = variational_topic_inference(ids, cts, exp_elog_beta, state.alpha, g0)
        np.add.at(stat.T, np.asarray(ids), sstats.T)
        logphat += dirichlet_expectation(gamma)
        iters.append(it)
    if n_nonempty == 0:
        return {"n_nonempty": 0, "iters": iters}
    batch_result = stat * exp_elog_beta.T
    batch_size = int(math.ceil(state.mini_batch_fraction * state.corpus_size))
    update_lambda(state, batch_result, batch_size)
    if state.optimize_doc_concentration:
        update_alpha(state, logphat / n_nonempty, n_nonempty)
    return {"n_nonempty": n_nonempty, "iters": iters, "logphat": logphat, "stat": stat}


def update_lambda(state: OnlineLDAState, stat, batch_size):
    """[U] updateLambda: λ ← (1−ρ)λ + ρ(stat·D/batchSize + η)."""
    w = state.rho()
    state.lam = (1 - w) * state.lam + w * (stat * (state.corpus_size / batch_size) + state.eta)


def update_alpha(state: OnlineLDAState, logphat, n):
    """[U] updateAlpha: one Newton step on α (Blei/Hoffman), applied only if α stays > 0."""
    w = state.rho()
    alpha = state.alpha
    gradf = n * (-dirichlet_expectation(alpha) + logphat)
    c = n * trigamma(np.array([alpha.sum()]))[0]
    q = -n * trigamma(alpha)
    b = np.sum(gradf / q) / (1.0 / c + np.sum(1.0 / q))
    dalpha = -(gradf - b) / q
    if np.all(w * dalpha + alpha > 0):
        state.alpha = alpha + w * dalpha


# ---------------------------------------------------------------------------------------
# LocalLDAModel   [U] mllib.clustering.LocalLDAModel
# ---------------------------------------------------------------------------------------
def topics_exp_elog_beta(topics_matrix):
    """exp(dirichletExpectation(topicsMatrixᵀ))ᵀ for a V×k topicsMatrix."""
    return np.exp(dirichlet_expectation(np.asarray(topics_matrix).T)).T


def topic_distribution(ids, cts, topics_matrix, alpha, gamma0, exp_elog_beta=None):
    """[U] LocalLDAModel.topicDistribution (LDALoader.scala:108): E-step → γ/‖γ‖₁."""
    k = np.asarray(alpha).size
    if len(ids) == 0:
        return np.zeros(k)
    eeb = topics_exp_elog_beta(topics_matrix) if exp_elog_beta is None else exp_elog_beta
    gamma, _, _ = variational_topic_inference(ids, cts, eeb, alpha, gamma0)
    return gamma / np.abs(gamma).sum()


def doc_bound(ids, cts, elog_beta, alpha, gamma):
    """One document's four terms of [U] LocalLDAModel.logLikelihoodBound from a given γ:
    Σ_w cnt_w·logSumExp(E[log θ] + E[log β_w]) + Σ(α − γ)·E[log θ] + Σ(lgamma γ − lgamma α)
    + lgamma Σα − lgamma Σγ.  elog_beta is V×k.  Entries with cts == 0 are skipped (their term is 0·x).
    The token terms are added in entry order, as upstream's foreachActive adds them."""
    ids = np.asarray(ids)
    cts = np.asarray(cts, np.float64)
    alpha = np.asarray(alpha, np.float64)
    gamma = np.asarray(gamma, np.float64)
    elog_theta = dirichlet_expectation(gamma)
    nz = cts != 0
    b = 0.0
    if nz.any():
        x = elog_beta[ids[nz]] + elog_theta                  # nnz × k
        a = x.max(axis=1)
        lse = a + np.log(np.exp(x - a[:, None]).sum(axis=1))
        for t in (cts[nz] * lse).tolist():
            b += t
    b += np.sum((alpha - gamma) * elog_theta)
    b += np.sum(gammaln(gamma) - gammaln(alpha))
    b += gammaln(alpha.sum()) - gammaln(gamma.sum())
    return b


def topics_bound(topics_matrix, eta, elog_beta=None):
    """[U] logLikelihoodBound's topicsPart E[log p(β|η) − log q(β|λ)]: Σ(η−λ)·Elogβ + Σ(lgamma λ − lgamma η)
    + Σ_k (lgamma(Vη) − lgamma Σ_v λ_vk)   (upstream: `sum(lgamma(sumEta) - lgamma(sum(lambda(::,
    breeze.linalg.*))))`, λ = topicsMatrix V×k).  elog_beta: dirichlet_expectation(λᵀ)ᵀ if the caller has it."""
    lam = np.asarray(topics_matrix, np.float64)
    if elog_beta is None:
        elog_beta = dirichlet_expectation(lam.T).T
    sum_eta = eta * lam.shape[0]
    return (np.sum((eta - lam) * elog_beta) + np.sum(gammaln(lam) - gammaln(eta))
            + np.sum(gammaln(sum_eta) - gammaln(lam.sum(axis=0))))


def log_likelihood_bound(docs, gamma0s, topics_matrix, alpha, eta):
    """[U] LocalLDAModel.logLikelihoodBound: corpusPart + topicsPart (ELBO).

    docs: list of (ids, cts); topics_matrix: V×k (λᵀ).  Returns (bound, corpus_part, topics_part).
    """
    lam = np.asarray(topics_matrix, np.float64)          # V × k
    V, k = lam.shape
    alpha = np.asarray(alpha, np.float64)
    elog_beta = dirichlet_expectation(lam.T).T           # V × k
    eeb = np.exp(elog_beta)
    corpus = 0.0
    for (ids, cts), g0 in zip(docs, gamma0s):
        if len(ids) == 0 or not np.any(np.asarray(cts) != 0):
            continue
        gamma, _, _ = variational_topic_inference(ids, cts, eeb, alpha, g0)
        corpus += doc_bound(ids, cts, elog_beta, alpha, gamma)
    topics = topics_bound(lam, eta, elog_beta)
    return corpus + topics, corpus, topics


def log_perplexity(docs, gamma0s, topics_matrix, alpha, eta):
    """[U] LocalLDAModel.logPerplexity: −bound / Σ token counts."""
    tokens = sum(float(np.sum(c)) for _, c in docs)
    return -log_likelihood_bound(docs, gamma0s, topics_matrix, alpha, eta)[0] / tokens


def describe_topics(topics_matrix, max_terms_per_topic=10):
    """[U] LocalLDAModel.describeTopics: per topic L1-normalise the column, stable sort by −w.

    Returns (indices k×N int64, weights k×N float64).  Ties keep ascending term index
    (Scala's sortBy is stable over zipWithIndex).
    """
    lam = np.asarray(topics_matrix, np.float64)
    V, k = lam.shape
    n = min(max_terms_per_topic, V)
    idx = np.zeros((k, n), np.int64)
    w = np.zeros((k, n))
    for t in range(k):
        col = lam[:, t] / np.abs(lam[:, t]).sum()
        order = np.argsort(-col, kind="stable")[:n]
        idx[t] = order
        w[t] = col[order]
    return idx, w
