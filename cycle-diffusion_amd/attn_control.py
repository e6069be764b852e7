"""Host side of the cross-attention control (prompt-to-prompt, Hertz et al. 2022, on the coupled translate loop).

build_control() turns the token ids of a source and a target prompt into what cd_cycle_translate's cd_attn_ctrl consumes:
    M [B, L, L]   mapper: (P_src . M)[j] = sum_i P_src[i] M[i, j] - the source attention map seen from target position j
    alpha [B, L]  1 where target position j takes the mapped source map, 0 where it keeps its own
    w [B, L]      re-weighting of target position j (1 = unchanged)
It works on id arrays, not on strings: any tokenizer that pads to a fixed length and marks the end of the prompt with one id
will do (the CLIP BPE, the BERT WordPiece and the hash stand-ins of gan_wrapper/text_encoders.py).

word_selector() / edited_selector() build the key-position selectors of the per-word attention maps (cd_word_maps, DESIGN.md
17) from the same id arrays, and blend_mask() turns such maps into a keep-mask by prompt-to-prompt's LocalBlend rule.

The alignment is the global (Needleman-Wunsch) alignment of prompt-to-prompt's seq_aligner: match +1, gap 0, mismatch -1,
ties resolved in its order (gap in the source, gap in the target, diagonal). With these scores a substituted token never
aligns diagonally (two gaps score 0 > -1): it shows up as one source token left out and one target token inserted.
"""
import numpy as np

CLIP_EOS = 49407
MODES = ("refine", "replace")


def prompt_length(ids, eos_id):
    """index of the end token of one padded id row (its last position when the row has none)"""
    hit = np.nonzero(np.asarray(ids) == eos_id)[0]
    return int(hit[0]) if len(hit) else len(ids) - 1


def align(src, tgt):
    """Needleman-Wunsch (match 1, gap 0, mismatch -1) -> for every target token the index of the source token it is aligned
    with, or -1 for an inserted one. Aligned pairs are not necessarily equal tokens in general; with these scores they are."""
    n, m = len(src), len(tgt)
    score = np.zeros((n + 1, m + 1), dtype=np.int64)
    trace = np.zeros((n + 1, m + 1), dtype=np.int8)
    trace[0, 1:] = 1
    trace[1:, 0] = 2
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            left, up = score[i, j - 1], score[i - 1, j]
            diag = score[i - 1, j - 1] + (1 if src[i - 1] == tgt[j - 1] else -1)
            best = max(left, up, diag)
            score[i, j] = best
            trace[i, j] = 1 if best == left else (2 if best == up else 3)
    out = [-1] * m
    i, j = n, m
    while i > 0 or j > 0:
        if trace[i, j] == 3:
            i, j = i - 1, j - 1
            out[j] = i
        elif trace[i, j] == 1:
            j -= 1
        else:
            i -= 1
    return out


def build_control(src_ids, tgt_ids, mode="refine", reweight=None, eos_id=CLIP_EOS):
    """src_ids, tgt_ids: integer arrays [B, L] (start token, prompt, end token, padding). Returns float32 (M [B, L, L],
    alpha [B, L], w [B, L]).
      refine   a target token aligned with an EQUAL source token takes that token's map (M[i, j] = 1, alpha_j = 1); inserted and
               substituted tokens keep their own attention (alpha_j = 0, column j of M empty)
      replace  the prompts must have the same number of tokens; every position takes the source map of the same position,
               substituted ones included (alpha_j = 1)
    In both modes the start token maps to the start token, and the positions from the target's end token onward map in order
    to the source positions from the source's end token onward (clipped to L - 1), alpha = 1.
    reweight: {key: scale}; a key below L is a target position, any other key a token id (every occurrence ahead of the
    target's end token); w is 1 elsewhere."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (MODES,))
    src_ids, tgt_ids = np.asarray(src_ids), np.asarray(tgt_ids)
    if src_ids.ndim != 2 or src_ids.shape != tgt_ids.shape:
        raise ValueError("src_ids and tgt_ids must both be [B, L], got %s and %s" % (src_ids.shape, tgt_ids.shape))
    B, L = src_ids.shape
    M = np.zeros((B, L, L), dtype=np.float32)
    alpha = np.zeros((B, L), dtype=np.float32)
    w = np.ones((B, L), dtype=np.float32)
    for b in range(B):
        s, t = src_ids[b], tgt_ids[b]
        ns, nt = prompt_length(s, eos_id), prompt_length(t, eos_id)
        M[b, 0, 0] = 1.0
        alpha[b, 0] = 1.0
        if mode == "replace":
            if ns != nt:
                raise ValueError("mode = 'replace' needs prompts of the same number of tokens (sample %d: %d against %d); "
                                 "use mode = 'refine'" % (b, ns - 1, nt - 1))
            for j in range(1, nt):
                M[b, j, j] = 1.0
                alpha[b, j] = 1.0
        else:
            for jj, ii in enumerate(align(list(s[1:ns]), list(t[1:nt]))):
                if ii >= 0 and s[1 + ii] == t[1 + jj]:
                    M[b, 1 + ii, 1 + jj] = 1.0
                    alpha[b, 1 + jj] = 1.0
        for k in range(L - nt):
            M[b, min(ns + k, L - 1), nt + k] = 1.0
            alpha[b, nt + k] = 1.0
        for key, scale in (reweight or {}).items():
            key = int(key)
            if 0 <= key < L:
                w[b, key] = float(scale)
            else:
                w[b, 1:nt][t[1:nt] == key] = float(scale)
    return M, alpha, w


# ------------------------------------------------------------------------------------------------ per-word attention maps
MAX_WORDS = 8  # selector rows of one cd_word_maps call (csrc/kernels.h kMapWords)


def word_selector(ids, words, eos_id=CLIP_EOS):
    """ids: one padded id row [L]; words: N token-id sequences (one word may be several tokens). Returns float32 [N, L]: row n
    is 1 at every position of every occurrence of words[n] between the start token and the end token, 0 elsewhere."""
    ids = np.asarray(ids)
    if ids.ndim != 1:
        raise ValueError("ids must be one id row [L], got %s" % (ids.shape,))
    words = [[int(t) for t in np.atleast_1d(np.asarray(w))] for w in words]
    if not 1 <= len(words) <= MAX_WORDS:
        raise ValueError("a selector holds 1 to %d words, got %d" % (MAX_WORDS, len(words)))
    end = prompt_length(ids, eos_id)
    sel = np.zeros((len(words), len(ids)), dtype=np.float32)
    for n, w in enumerate(words):
        for at in range(1, end - len(w) + 1):
            if len(w) and list(ids[at:at + len(w)]) == w:
                sel[n, at:at + len(w)] = 1.0
        if not sel[n].any():
            raise ValueError("word %d (tokens %s) does not occur in the prompt" % (n, w))
    return sel


def edited_selector(src_ids, tgt_ids, eos_id=CLIP_EOS):
    """src_ids, tgt_ids: one padded id row [L] each. Returns float32 [1, L]: 1 at the target positions align() does not pair
    with an equal source token - the words the edit introduces."""
    s, t = np.asarray(src_ids), np.asarray(tgt_ids)
    if s.ndim != 1 or s.shape != t.shape:
        raise ValueError("src_ids and tgt_ids must both be one id row [L], got %s and %s" % (s.shape, t.shape))
    ns, nt = prompt_length(s, eos_id), prompt_length(t, eos_id)
    sel = np.zeros((1, len(t)), dtype=np.float32)
    for jj, ii in enumerate(align(list(s[1:ns]), list(t[1:nt]))):
        if ii < 0 or s[1 + ii] != t[1 + jj]:
            sel[0, 1 + jj] = 1.0
    if not sel.any():
        raise ValueError("the target prompt introduces no token: every one is aligned with an equal source token")
    return sel


def blend_mask(maps, threshold=0.3, pool=3, factor=1):
    """prompt-to-prompt's LocalBlend rule on maps [B, N, h, w] (a torch tensor): sum over the words, max_pool2d(pool, 1,
    pool // 2), divide by the image's own maximum (an all-zero image edits nothing), edit = value > threshold. Returns the
    keep-mask 1 - edit as float32 [B, 1, h * factor, w * factor] by nearest replication: the orientation and form
    translate(mask=) takes (1 = keep the source)."""
    import torch
    import torch.nn.functional as F
    if maps.dim() != 4:
        raise ValueError("maps must be [B, N, h, w], got %s" % (tuple(maps.shape),))
    if pool < 1 or pool % 2 != 1 or int(factor) < 1:
        raise ValueError("pool must be odd and >= 1, factor >= 1; got pool = %s, factor = %s" % (pool, factor))
    m = maps.float().sum(1, keepdim=True)
    m = F.max_pool2d(m, pool, 1, pool // 2)
    mx = m.amax(dim=(1, 2, 3), keepdim=True)
    m = torch.where(mx > 0, m / mx.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(m))
    keep = 1.0 - (m > threshold).float()
    return keep.repeat_interleave(int(factor), 2).repeat_interleave(int(factor), 3).contiguous()


# ------------------------------------------------------------------------------------------------ local blend
LOCAL_BLEND_MODES = ("none", "words")


def local_blend_selectors(src_ids, tgt_ids, eos_id=CLIP_EOS, words=None):
    """The selectors of the local blend (cd_local_blend) for one sample: (sel_src [L], sel_tgt [L]) float32. Without `words`:
    edited_selector both ways - the target positions not paired with an equal source token, and the source positions not
    paired with an equal target token; a side that has none (an insertion leaves the source without one, identical prompts
    leave both) is all zero, and an all-zero map edits nothing. words = (src_words, tgt_words): token-id sequences marked by
    word_selector in their own prompt (an empty list: zero), their rows summed."""
    s, t = np.asarray(src_ids), np.asarray(tgt_ids)
    if s.ndim != 1 or s.shape != t.shape:
        raise ValueError("src_ids and tgt_ids must both be one id row [L], got %s and %s" % (s.shape, t.shape))
    if words is not None:
        out = []
        for row, ws in ((s, words[0]), (t, words[1])):
            ws = list(ws)
            out.append(np.minimum(word_selector(row, ws, eos_id).sum(0), 1.0).astype(np.float32) if ws
                       else np.zeros(len(row), dtype=np.float32))
        return out[0], out[1]

    def one(a, b):  # the positions of b that a does not explain
        try:
            return edited_selector(a, b, eos_id)[0]
        except ValueError:
            return np.zeros(len(b), dtype=np.float32)

    return one(t, s), one(s, t)


def local_blend_start(fraction, K):
    """n_start of a member that runs K decode steps: the blend begins after the first int(fraction * K) iterations"""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("local_blend_start must lie in [0, 1] (the unblended fraction of the decode steps), got %r" % (fraction,))
    return int(float(fraction) * int(K))


LOCAL_BLEND_KEYS = ("local_blend", "local_blend_threshold", "local_blend_pool", "local_blend_side", "local_blend_start")


def refuse_local_blend(kw, who):
    """wrappers without the coupled text loop refuse the local blend's keys by name (removed from `kw` either way)"""
    got = {k: kw.pop(k) for k in LOCAL_BLEND_KEYS if k in kw}
    given = sorted(k for k, v in got.items() if v is not None and not (k == "local_blend" and str(v) == "none"))
    if given:
        raise ValueError("%s does not use %s: the local blend needs the source rows of the coupled translate loop of the latent "
                         "text wrappers (SDStochasticText / LatentDiffStochasticText); remove %s from the [gan] section"
                         % (who, ", ".join(given), "it" if len(given) == 1 else "them"))
