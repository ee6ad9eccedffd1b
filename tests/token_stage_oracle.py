"""Plain-Python restatement of the token stages (include/stc.h, "Token stages"): what the kernels of
token_stages.hip must compute, token for token.

swr    [U] ml.feature.StopWordsRemover.transform: case-sensitive — drop the tokens whose bytes are in the list;
       case-insensitive — drop the tokens whose Java 8 root-locale lower case (oracle.java_lower, applied to the token
       as a string of its own) is the lower case of a listed word.  Kept tokens are returned as they came.
ngram  [U] ml.feature.NGram: sliding(n).withPartial(false).map(_.mkString(" ")).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.oracle import java_lower  # noqa: E402


def _bytes(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def swr(docs, stop, case_sensitive):
    """docs: list[list[str]] (str | bytes when case_sensitive) → the same with the stop words dropped"""
    if case_sensitive:
        drop = {_bytes(w) for w in stop}
        return [[t for t in d if _bytes(t) not in drop] for d in docs]
    drop = {java_lower(w) for w in stop}
    return [[t for t in d if java_lower(t) not in drop] for d in docs]


def ngram(docs, n):
    """docs: list[list[str]] → every run of n consecutive tokens of a document joined by one space"""
    if n < 1:
        raise ValueError(f"n must be >= 1 but got {n}")
    return [[" ".join(d[i:i + n]) for i in range(len(d) - n + 1)] for d in docs]
