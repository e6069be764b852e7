"""The `[gan] auto_mask*` keys: a keep-mask estimated from the two prompts (DiffEdit, Couairon et al. 2022, step 1; DESIGN.md
16) for the region-masked translation of the latent text wrappers. Host-side only: the keys, their ranges and the level of
the estimate; the estimate itself is cd_automask (Engine.automask).

  auto_mask           = none | diffedit   off (the default) or on
  auto_mask_draws     = 10                noised copies of the source latent the two predictions are compared on
  auto_mask_strength  = 0.5               how far the source is noised: level k = clamp(int(strength * S) - 1, 0, S - 1) of the
                                          wrapper's own S-step schedule
  auto_mask_ratio     = 3.0               the map is clipped at ratio x the image's own mean, then scaled to [0, 1]
  auto_mask_threshold = 0.5               edit where the scaled map exceeds it
  auto_mask_dilate    = 0                 the edit region grows by this many latent pixels (<= 8)
  auto_mask_seed      = 0                 seed of the estimate's own draws (counter-based generator, streams STREAM0 + i)
"""
MODES = ("none", "diffedit")
KEYS = ("auto_mask", "auto_mask_draws", "auto_mask_strength", "auto_mask_ratio", "auto_mask_threshold", "auto_mask_dilate",
        "auto_mask_seed")
STREAM0 = 0x6000     # draw i of the estimate is Philox stream STREAM0 + i
MAX_DRAWS = 0xFFF    # the width of a stream band
MAX_DILATE = 8


class AutoMaskOptions:
    def __init__(self, auto_mask=None, auto_mask_draws=10, auto_mask_strength=0.5, auto_mask_ratio=3.0,
                 auto_mask_threshold=0.5, auto_mask_dilate=0, auto_mask_seed=0):
        mode = "none" if auto_mask is None else str(auto_mask)  # a config's `none` arrives as None
        if mode not in MODES:
            raise ValueError("auto_mask must be one of %s, got %r" % (MODES, auto_mask))
        for name, v in (("auto_mask_draws", auto_mask_draws), ("auto_mask_dilate", auto_mask_dilate),
                        ("auto_mask_seed", auto_mask_seed)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError("%s must be an integer, got %r" % (name, v))
        if not 1 <= auto_mask_draws <= MAX_DRAWS:
            raise ValueError("auto_mask_draws must lie in [1, %d], got %r" % (MAX_DRAWS, auto_mask_draws))
        if not 0.0 < float(auto_mask_strength) <= 1.0:
            raise ValueError("auto_mask_strength must lie in (0, 1], got %r" % (auto_mask_strength,))
        if not float(auto_mask_ratio) > 0.0:
            raise ValueError("auto_mask_ratio must be > 0, got %r" % (auto_mask_ratio,))
        if not 0.0 <= float(auto_mask_threshold) < 1.0:
            raise ValueError("auto_mask_threshold must lie in [0, 1), got %r" % (auto_mask_threshold,))
        if not 0 <= auto_mask_dilate <= MAX_DILATE:
            raise ValueError("auto_mask_dilate must lie in [0, %d], got %r" % (MAX_DILATE, auto_mask_dilate))
        if not 0 <= auto_mask_seed < 2 ** 64:
            raise ValueError("auto_mask_seed must fit 64 bits, got %r" % (auto_mask_seed,))
        self.mode, self.draws, self.strength = mode, int(auto_mask_draws), float(auto_mask_strength)
        self.ratio, self.threshold = float(auto_mask_ratio), float(auto_mask_threshold)
        self.dilate, self.seed = int(auto_mask_dilate), int(auto_mask_seed)

    @property
    def on(self):
        return self.mode != "none"


def level_index(strength, steps):
    """row k of the schedule's tables the estimate noises to: clamp(int(strength * S) - 1, 0, S - 1)"""
    return max(0, min(int(steps) - 1, int(float(strength) * int(steps)) - 1))


def pop_keys(kw):
    """the auto_mask* entries of a kwargs dict, removed from it"""
    return {k: kw.pop(k) for k in KEYS if k in kw}


def refuse(kw, who):
    """wrappers without a keep-mask refuse the keys by name (removed from `kw` either way)"""
    given = sorted(k for k, v in pop_keys(kw).items() if v is not None and not (k == "auto_mask" and str(v) == "none"))
    if given:
        raise ValueError("%s takes no %s: the keep-mask estimate belongs to the region-masked translation of the latent text "
                         "wrappers (SDStochasticText / LatentDiffStochasticText); remove %s from the [gan] section"
                         % (who, ", ".join(given), "it" if len(given) == 1 else "them"))
