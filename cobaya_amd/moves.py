"""The option `moves`: a weighted mixture of ensemble moves ("Ensemble move
mixtures"; mcmc_hip_set_moves).  A list of 1 .. 8 members, each `[kind, weight]` or
`[kind, weight, {params}]`:

    "stretch"   a      (2.0)                      the stretch move
    "de"        gamma  (None: 2.38 / sqrt(2 d)),  sigma (1e-5)    differential evolution
    "snooker"   gamma  (1.7)                      the snooker update

`parse` turns it into the arrays of the C entry, naming whatever it refuses; sampler and engine both
go through it, so they refuse alike."""
import math

ENSEMBLE_STRETCH, ENSEMBLE_DE, ENSEMBLE_SNOOKER = 0, 1, 2   # mcmc_hip.h: MCMC_HIP_ENSEMBLE_*
MAX_MOVES = 8
KINDS = {"stretch": ENSEMBLE_STRETCH, "de": ENSEMBLE_DE, "snooker": ENSEMBLE_SNOOKER}
NAMES = {v: k for k, v in KINDS.items()}
PARAMS = {"stretch": {"a": 2.0}, "de": {"gamma": None, "sigma": 1e-5}, "snooker": {"gamma": 1.7}}


def _number(where, name, value):
    if isinstance(value, bool):
        raise ValueError("%s: %s must be a number, got %r" % (where, name, value))
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a number, got %r" % (where, name, value)) from None


def parse(moves, d):
    """[(kind id, weight as given, p0, p1)] of the members; ValueError names the offender."""
    if not isinstance(moves, (list, tuple)) or not 1 <= len(moves) <= MAX_MOVES:
        raise ValueError("moves must be a list of 1 .. %d members [kind, weight] or [kind, weight, {params}], got %r"
                         % (MAX_MOVES, moves))
    out = []
    for j, member in enumerate(moves):
        where = "moves[%d]" % j
        if not isinstance(member, (list, tuple)) or len(member) not in (2, 3):
            raise ValueError("%s must be [kind, weight] or [kind, weight, {params}], got %r" % (where, member))
        kind, weight = member[0], _number(where, "the weight", member[1])
        if kind not in KINDS:
            raise ValueError("%s: unknown kind %r (the kinds are 'stretch', 'de' and 'snooker')" % (where, kind))
        where = "%s (%s)" % (where, kind)
        if not (math.isfinite(weight) and weight > 0):
            raise ValueError("%s: the weight must be positive and finite, got %r" % (where, weight))
        given = member[2] if len(member) == 3 and member[2] is not None else {}
        if not isinstance(given, dict):
            raise ValueError("%s: the parameters must be a dict, got %r" % (where, given))
        unknown = sorted(set(given) - set(PARAMS[kind]))
        if unknown:
            raise ValueError("%s: unknown parameter %r (it has %s)" % (where, unknown[0], sorted(PARAMS[kind])))
        par = {**PARAMS[kind], **given}
        if kind == "stretch":
            p0, p1 = _number(where, "a", par["a"]), 0.0
            if not (math.isfinite(p0) and p0 > 1):
                raise ValueError("%s: a must be finite and > 1, got %r" % (where, p0))
        else:
            p0 = 2.38 / math.sqrt(2 * d) if par["gamma"] is None else _number(where, "gamma", par["gamma"])
            if not (math.isfinite(p0) and p0 > 0):
                raise ValueError("%s: gamma must be finite and > 0, got %r" % (where, p0))
            p1 = _number(where, "sigma", par["sigma"]) if kind == "de" else 0.0
            if not (math.isfinite(p1) and p1 >= 0):
                raise ValueError("%s: sigma must be finite and >= 0, got %r" % (where, p1))
        out.append((KINDS[kind], weight, p0, p1))
    return out


def normalised(members):
    """The members with their weights divided by the ascending sum, as mcmc_hip_set_moves divides."""
    total = 0.0
    for _, w, _, _ in members:
        total += w
    return [(k, w / total, p0, p1) for k, w, p0, p1 in members]


def describe(rows):
    """One line for a table of (kind, weight, p0, p1) rows (the state file's)."""
    def one(k, w, p0, p1):
        name = NAMES.get(int(k), "?")
        par = {"stretch": "a: %g" % p0, "de": "gamma: %g, sigma: %g" % (p0, p1), "snooker": "gamma: %g" % p0}.get(name, "")
        return "%s %.4g (%s)" % (name, w, par)
    return "[" + ", ".join(one(*r) for r in rows) + "]"
