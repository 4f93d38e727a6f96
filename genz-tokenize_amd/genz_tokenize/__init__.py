"""MI355X-native drop-in for the tokenizer of DVNghiem/genz-tokenize (reference genz_tokenize/__init__.py:1-10
exports `Tokenize`).  `genz_tokenize.preprocess` mirrors the reference's text filters and `genz_tokenize.ranking` its BM25 /
BM25Plus, both on the GPU; `genz_tokenize.learn` makes the merges and the vocabulary `Tokenize.fromFile` takes from a corpus; the
reference's `models` sub-package is out of scope, see DESIGN.md."""
from .tokenize import NgramIndex, Tokenize, get_pairs  # noqa: F401
from .learn import learn_bpe, word_counts  # noqa: F401

__all__ = ['Tokenize', 'NgramIndex', 'get_pairs', 'learn_bpe', 'word_counts']
__version__ = '1.2.7+mi355x.1'
