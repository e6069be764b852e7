"""Semantic guidance (SEGA; Brack et al., NeurIPS 2023) on the coupled translate loop: the host side.

An edit concept is a text with its own signed scale, quantile threshold, weight and window of iterations. This module holds
the concept itself, the grammar of the `[gan] edit_concepts` string and the table the engine takes
(include/cyclediff.h cd_sega_concept): the quantile q over the N values of a latent becomes, in float64, the rank
lo = floor(q (N - 1)) and the weight frac = q (N - 1) - lo of the two order statistics it lies between. Everything the engine
would refuse is raised here first, as ValueError.
"""
import math
from dataclasses import dataclass

import numpy as np

from . import _ffi

MAX_CONCEPTS = 8


@dataclass
class EditConcept:
    text: str
    scale: float = 5.0       # guidance scale of the concept, >= 0; the direction comes from `reverse`
    threshold: float = 0.9   # quantile of |d| below which an element is left alone
    reverse: bool = False    # steer away from the concept
    warmup: float = 0.1      # fraction of the loop before the concept acts
    cooldown: float = 1.0    # fraction of the loop after which it no longer acts
    weight: float = 1.0      # weight in the sum over concepts


def parse_concepts(spec):
    """"+glasses:5:0.9; -smile" -> [EditConcept]. Items are separated by ';', each `[+|-]text[:scale[:threshold]]`, '-' meaning
    reverse. An empty string is no concept."""
    out = []
    if spec is None or not str(spec).strip():
        return out
    for item in str(spec).split(";"):
        item = item.strip()
        if not item:
            raise ValueError("edit_concepts: empty item in %r" % (spec,))
        reverse = item[0] == "-"
        if item[0] in "+-":
            item = item[1:]
        parts = [p.strip() for p in item.split(":")]
        if len(parts) > 3:
            raise ValueError("edit_concepts: %r has more than text:scale:threshold" % (item,))
        if not parts[0]:
            raise ValueError("edit_concepts: an item of %r has no text" % (spec,))
        kw = {}
        try:
            if len(parts) > 1:
                kw["scale"] = float(parts[1])
            if len(parts) > 2:
                kw["threshold"] = float(parts[2])
        except ValueError:
            raise ValueError("edit_concepts: scale / threshold of %r is not a number" % (item,))
        out.append(EditConcept(parts[0], reverse=reverse, **kw))
    check_concepts(out)
    return out


def check_concepts(concepts, momentum_scale=0.0, momentum_beta=0.0):
    """what can be refused without the loop's length: each refusal of semantic guidance (cd_sega) that concerns the concepts"""
    if not 1 <= len(concepts) <= MAX_CONCEPTS:
        raise ValueError("semantic guidance takes 1 to %d concepts, got %d" % (MAX_CONCEPTS, len(concepts)))
    for c in concepts:
        if not isinstance(c.text, str) or not c.text.strip():
            raise ValueError("an edit concept needs a text")
        for name in ("scale", "weight", "threshold", "warmup", "cooldown"):
            if not math.isfinite(float(getattr(c, name))):
                raise ValueError("edit concept %r: %s is not finite" % (c.text, name))
        if c.scale < 0:
            raise ValueError("edit concept %r: scale %g is negative (reverse=True steers away)" % (c.text, c.scale))
        if not 0.0 <= c.threshold <= 1.0:
            raise ValueError("edit concept %r: threshold %g outside [0, 1]" % (c.text, c.threshold))
        if not 0.0 <= c.warmup <= c.cooldown <= 1.0:
            raise ValueError("edit concept %r: warmup %g / cooldown %g outside 0 <= warmup <= cooldown <= 1"
                             % (c.text, c.warmup, c.cooldown))
    for name, v in (("edit_momentum_scale", momentum_scale), ("edit_momentum_beta", momentum_beta)):
        if not math.isfinite(float(v)):
            raise ValueError("%s is not finite" % name)
    if not 0.0 <= momentum_beta <= 1.0:
        raise ValueError("edit_momentum_beta %g outside [0, 1]" % momentum_beta)


def quantile_rank(q, N):
    """(lo, frac) of the quantile q over N values: lo = floor(q (N - 1)), frac = float32(q (N - 1) - lo), in float64"""
    pos = float(q) * (int(N) - 1)
    lo = min(int(math.floor(pos)), int(N) - 1)
    frac = float(np.float32(pos - lo))
    if frac >= 1.0:  # a weight that rounds to 1 in float32: the next order statistic itself (lo < N - 1 here)
        lo, frac = lo + 1, 0.0
    return lo, frac


def table_rows(rows, K, N):
    """(scale, weight, q, warm, cool) per concept, scale signed -> the cd_sega_concept array; the engine's refusals of a row"""
    if not 1 <= len(rows) <= MAX_CONCEPTS:
        raise ValueError("semantic guidance takes 1 to %d concepts, got %d" % (MAX_CONCEPTS, len(rows)))
    if int(N) < 1 or int(K) < 1:
        raise ValueError("semantic guidance: K = %d steps over N = %d values" % (K, N))
    tab = np.zeros(len(rows), dtype=_ffi.SEGA_CONCEPT_DTYPE)
    for e, (scale, weight, q, warm, cool) in enumerate(rows):
        if not (math.isfinite(scale) and math.isfinite(weight)):
            raise ValueError("concept %d: scale / weight is not finite" % e)
        if not 0.0 <= q <= 1.0:
            raise ValueError("concept %d: threshold %g outside [0, 1]" % (e, q))
        if not 0 <= warm <= cool <= K:
            raise ValueError("concept %d: warm = %d / cool = %d outside 0 <= warm <= cool <= K = %d" % (e, warm, cool, K))
        lo, frac = quantile_rank(q, N)
        tab[e] = (scale, weight, lo, frac, warm, cool)
    return tab


def concept_table(concepts, K, N):
    """[EditConcept] -> the cd_sega_concept rows for a loop of K iterations over latents of N = C*H*W values:
    warm = int(warmup K), cool = int(cooldown K), scale signed by `reverse`"""
    check_concepts(concepts)
    return table_rows([((-1.0 if c.reverse else 1.0) * float(c.scale), float(c.weight), float(c.threshold),
                        int(c.warmup * K), int(c.cooldown * K)) for c in concepts], K, N)


KEYS = ("edit_concepts", "edit_momentum_scale", "edit_momentum_beta")


def refuse(kw, who):
    """wrappers without the coupled text loop refuse the [gan] keys of semantic guidance by name (removed from `kw` either way)"""
    got = {k: kw.pop(k) for k in KEYS if k in kw}
    given = sorted(k for k, v in got.items() if v is not None and not (k == "edit_concepts" and not str(v).strip()))
    if given:
        raise ValueError("%s does not use %s: remove %s from the [gan] section" % (who, ", ".join(given),
                                                                                  "it" if len(given) == 1 else "them"))
