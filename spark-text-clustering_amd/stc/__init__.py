"""stc — MI355X-native text preprocessing → HashingTF / CountVectorizer → IDF → LDA (online and EM) hot path of borisfoko/Spark-Text-Clustering.

The compute lives in libstc.so (HIP kernels for gfx950 behind the C ABI in include/stc.h); this
package is the host-side mirror of the Spark ML interface the reference's pipeline uses.
"""
from ._lib import (STC_ERR_HIP, STC_ERR_INVALID_ARG, STC_ERR_OOM, STC_ERR_RCCL, STC_ERR_STATE, STC_F32, STC_F64, STC_MIXED,
                   STC_HASH_SPARK24, STC_HASH_STANDARD, STC_LAYOUT_KV, STC_LAYOUT_VK, StcError, StcIllegalArgument,
                   load)
from . import io
from .clustering import (LDA, ML_LDA_DEFAULT_SEED, DistributedLDAModel, DocumentScores, EmGroup, EmHandle, EMLDAOptimizer, LdaGroup,
                         LdaHandle, LDAModel, MllibLDA, OnlineLDAOptimizer, em_concentrations,
                         reference_mini_batch_fraction)
from .coherence import coherence, term_cooccurrence
from .core import Context, CsrMatrix, DeviceCsr
from .count_vectorizer import CountVectorizer, CountVectorizerModel
from .feature import IDF, DeviceTokens, HashingTF, IDFModel, Tokenizer, encode_texts, encode_tokens
from .text_prep import DEFAULT_STRIP_CHARS, PorterStemmer, TextPreprocessor
from .token_stages import NGram, StopWordsRemover

__all__ = [
    "Context", "CsrMatrix", "DeviceCsr", "CountVectorizer", "CountVectorizerModel", "HashingTF", "IDF", "IDFModel", "Tokenizer", "DeviceTokens", "TextPreprocessor", "StopWordsRemover", "NGram", "PorterStemmer", "DEFAULT_STRIP_CHARS", "encode_texts", "encode_tokens", "LDA",
    "LDAModel", "DistributedLDAModel", "DocumentScores", "LdaGroup", "LdaHandle", "EmHandle", "EmGroup", "io", "MllibLDA", "OnlineLDAOptimizer",
    "EMLDAOptimizer", "em_concentrations", "ML_LDA_DEFAULT_SEED", "reference_mini_batch_fraction", "StcError", "StcIllegalArgument", "load", "STC_F32", "STC_F64", "STC_MIXED",
    "STC_HASH_STANDARD", "STC_HASH_SPARK24", "STC_LAYOUT_VK", "STC_LAYOUT_KV", "STC_ERR_INVALID_ARG", "STC_ERR_HIP",
    "STC_ERR_RCCL", "STC_ERR_OOM", "STC_ERR_STATE", "coherence", "term_cooccurrence",
]
