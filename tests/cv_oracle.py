"""Plain-Python restatement of CountVectorizer's semantics ([U] ml.feature.CountVectorizer, Spark 2.4.3) as
include/stc.h states them for stc_cv_*: dicts, and ``sorted`` on ``bytes`` (unsigned bytewise order, a
proper prefix first) for the ties of the term count.  Documents are lists of ``bytes`` (``str`` is encoded
as UTF-8).  The GPU tests compare against it exactly.
"""
import numpy as np

DEFAULT_VOCAB_SIZE = 1 << 18
DEFAULT_MAX_DF = float(2 ** 63 - 1)
EMPTY_MESSAGE = "The vocabulary size should be > 0. Lower minDF as necessary."


def as_bytes(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def fit(docs, vocabSize=DEFAULT_VOCAB_SIZE, minDF=1.0, maxDF=DEFAULT_MAX_DF):
    """→ (vocabulary list[bytes], counts int64, df int64); ValueError where the library returns
    STC_ERR_INVALID_ARG."""
    if vocabSize <= 0 or not minDF >= 0 or not maxDF >= 0:
        raise ValueError("vocabSize must be > 0, minDF and maxDF >= 0")
    n_docs = len(docs)
    min_df = float(minDF) if minDF >= 1.0 else float(minDF) * n_docs
    max_df = float(maxDF) if maxDF >= 1.0 else float(maxDF) * n_docs
    if max_df < min_df:
        raise ValueError("maxDF must be >= minDF")
    count, df = {}, {}
    for doc in docs:
        seen = set()
        for t in doc:
            t = as_bytes(t)
            count[t] = count.get(t, 0) + 1
            seen.add(t)
        for t in seen:
            df[t] = df.get(t, 0) + 1
    kept = [t for t in count if min_df <= float(df[t]) <= max_df]
    vocab = sorted(kept, key=lambda t: (-count[t], t))[:vocabSize]
    if not vocab:
        raise ValueError(EMPTY_MESSAGE)
    return vocab, np.array([count[t] for t in vocab], np.int64), np.array([df[t] for t in vocab], np.int64)


def index_map(vocab):
    index = {}
    for i, t in enumerate(vocab):
        t = as_bytes(t)
        if t in index:
            raise ValueError(f"the vocabulary holds the term {t!r} more than once")
        index[t] = i
    return index


def transform(docs, vocab, minTF=1.0, binary=False):
    """→ (indptr int64, indices int32, values float64) of the n_docs × len(vocab) CSR"""
    index = index_map(vocab)
    indptr, indices, values = [0], [], []
    for doc in docs:
        counts = {}
        for t in doc:
            i = index.get(as_bytes(t))
            if i is not None:
                counts[i] = counts.get(i, 0) + 1
        eff = float(minTF) if minTF >= 1.0 else len(doc) * float(minTF)
        for i in sorted(counts):
            if float(counts[i]) >= eff:
                indices.append(i)
                values.append(1.0 if binary else float(counts[i]))
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(values, np.float64)


def indices_of(terms, vocab):
    index = index_map(vocab)
    return np.array([index.get(as_bytes(t), -1) for t in terms], np.int32)
