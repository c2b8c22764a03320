"""Hotword boosting: a list of phrases as the ``sequence_bias`` the on-device decoder takes (tw_generate_greedy_biased).

HF's ``SequenceBiasLogitsProcessor`` biases the LAST token of a sequence once the tokens before it have been produced; its docstring's
advice for a multi-token word is to "apply the bias to their prefixes" as well.  ``sequence_bias_for`` does exactly that: for every
phrase, in every spelling variant, every non-empty prefix of its token ids becomes a sequence with the same boost, so each token along
the phrase is pushed once the tokens before it were produced.
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple


def sequence_bias_for(tokenizer, phrases: Iterable[str], boost: float, variants: Sequence[str] = (" {}", "{}")
                      ) -> Dict[Tuple[int, ...], float]:
    """``{tuple of token ids: boost}`` for ``WhisperEngine.generate_greedy(sequence_bias=...)`` / ``generate(sequence_bias=...)``.

    For every phrase and every variant (``" {}"``: the word inside a sentence, ``"{}"``: at its start) the phrase is tokenised without
    special tokens and EVERY non-empty prefix of its ids maps to ``boost``, which is in natural-log units on the logits (a boost of
    ``b`` multiplies the token's odds by ``exp(b)`` at the steps where it applies).  A tuple reached twice - a shared prefix of two
    phrases, a variant that tokenises like another - keeps one entry, in the place it was first reached.

    What this is not: there is no refund.  A partial match that breaks off keeps the boosts its first tokens received, because taking
    them back needs hypotheses to be compared after the fact, i.e. beam search, and the decoder is greedy.  Choose a boost that tips
    close calls, not one that forces the first token of a phrase wherever it could start."""
    boost = float(boost)
    if boost != boost or boost in (float("inf"), float("-inf")):
        raise ValueError(f"boost must be finite, got {boost!r}")
    out: Dict[Tuple[int, ...], float] = {}
    for phrase in phrases:
        if not isinstance(phrase, str) or not phrase.strip():
            raise ValueError(f"a hotword is a non-empty string, got {phrase!r}")
        for variant in variants:
            ids = [int(t) for t in tokenizer.encode(variant.format(phrase.strip()), add_special_tokens=False)]
            for n in range(1, len(ids) + 1):
                out.setdefault(tuple(ids[:n]), boost)
    return out
