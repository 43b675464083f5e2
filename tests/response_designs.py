"""Structured response designs for the parity tests: plain numpy, seeded, no GPU.

The parity tests used to draw every response as an independent coin flip with independent holes, which gives every person
(almost) the same number of observed cells and every item (almost) the same number of respondents.  The designs here are what
assessments look like instead: responses from a 2PL with known item parameters (so y correlates with the latent), then holes
punched by a DESIGN -- booklets of very different length, persons without a response, items nobody saw, constant items.

Every function returns (y, facts): y a uint8 matrix of 0 / 1 / 255 (255 = missing) and facts a dict of what the design
promises about it.  tests/test_response_designs.py asserts every promise on the matrix itself."""
import numpy as np

MISSING = 255


def _responses(rng, N, J):
    """0 / 1 responses of N persons to J items from a 2PL: slopes 0.5-2, difficulties N(0, 1), abilities N(0, 1)."""
    a = 0.5 + 1.5 * rng.rand(J)
    b = rng.randn(J)
    theta = rng.randn(N)
    p = 1.0 / (1.0 + np.exp(-(a[None, :] * (theta[:, None] - b[None, :]))))
    return (rng.rand(N, J) < p).astype(np.uint8)


def describe(y):
    """What a response matrix looks like, measured on the matrix: the figures the designs' promises are checked against."""
    obs = y != MISSING
    per_person, per_item = obs.sum(1), obs.sum(0)
    ones = ((y == 1) & obs).sum(0)
    return {
        "missing": float((~obs).sum()) / float(max(1, y.size)),
        "n_missing": int((~obs).sum()),
        "min_obs": int(per_person.min()) if len(per_person) else 0,
        "max_obs": int(per_person.max()) if len(per_person) else 0,
        "obs_per_person": per_person,
        "empty_persons": np.flatnonzero(per_person == 0),
        "complete_persons": np.flatnonzero(per_person == y.shape[1]),
        "unanswered_items": np.flatnonzero(per_item == 0),
        "all_one_items": np.flatnonzero((per_item > 0) & (ones == per_item)),
        "all_zero_items": np.flatnonzero((per_item > 0) & (ones == 0)),
    }


def booklets(N, J, lens, sorted_rows, seed=0, starts=None, counts=None):
    """Every person sees ONE contiguous booklet.  Booklet k holds lens[k] items from starts[k] on (default: one behind the
    other from item 0 where they fit -- the items behind the last booklet are then in no booklet --, spread evenly over the
    items where they do not) and is given to counts[k] persons (default: equal shares, the remainder to the last booklet).
    sorted_rows = True orders the rows by booklet like a data file; False shuffles them, so that any 64 consecutive persons
    and any window of 4096 mix all lengths."""
    rng = np.random.RandomState(seed)
    lens = [int(v) for v in lens]
    K = len(lens)
    assert K >= 1 and all(0 < v <= J for v in lens)
    if starts is None:
        if sum(lens) <= J:
            starts = [int(v) for v in np.cumsum([0] + lens[:-1])]
        else:
            starts = [int(round(k * (J - lens[k]) / float(max(1, K - 1)))) for k in range(K)]
    assert all(0 <= s and s + v <= J for s, v in zip(starts, lens))
    if counts is None:
        counts = [N // K] * K
        counts[-1] += N - sum(counts)
    assert sum(counts) == N
    book = np.repeat(np.arange(K), counts)
    if not sorted_rows:
        book = book[rng.permutation(N)]
    y = _responses(rng, N, J)
    cols = np.arange(J)[None, :]
    lo, ln = np.asarray(starts)[book][:, None], np.asarray(lens)[book][:, None]
    y[(cols < lo) | (cols >= lo + ln)] = MISSING
    covered = np.zeros(J, dtype=bool)
    for s, v, c in zip(starts, lens, counts):
        if c > 0:
            covered[s:s + v] = True
    facts = {"design": "booklets", "sorted_rows": bool(sorted_rows), "lens": lens, "starts": list(starts), "counts": list(counts),
             "booklet_of": book, "min_obs": min(v for v, c in zip(lens, counts) if c > 0),
             "max_obs": max(v for v, c in zip(lens, counts) if c > 0),
             "unanswered_items": np.flatnonzero(~covered), "empty_persons": np.zeros(0, dtype=np.int64),
             "n_missing": int(N * J - sum(v * c for v, c in zip(lens, counts)))}
    facts["missing"] = facts["n_missing"] / float(N * J)
    return y, facts


def with_edges(y, facts=None, seed=0, empty_person=True, empty_block=None, complete_case=False, unanswered_item=True,
               constant_items=True, constant_persons=True):
    """Named edge rows / columns added to any design (a copy; y itself is left alone):

    empty_person      one person with no observed cell;
    empty_block       first row of 64 CONSECUTIVE persons with no observed cell (None: no such block) -- sorted to the end of
                      their 4096-person window, they fill a whole 64-slot list group;
    complete_case     one person who answered every item (then no item stays unanswered: not together with unanswered_item);
    unanswered_item   one more item nobody answered;
    constant_items    one item everybody who saw it answered 1, and one everybody answered 0 (two respondents at least);
    constant_persons  one person whose observed responses are all 1, and one all 0 (neither saw the opposite constant item).

    The returned facts name each of them; the counts are measured on the result."""
    if complete_case and unanswered_item:
        raise ValueError("a complete case answers every item: no item can stay unanswered beside it")
    rng = np.random.RandomState(seed)
    y = y.copy()
    N, J = y.shape
    out = dict(facts or {})
    taken = np.zeros(N, dtype=bool)

    def pick_person(ok):
        cand = np.flatnonzero(ok & ~taken)
        if len(cand) == 0:
            raise ValueError("no person left for this edge")
        i = int(cand[rng.randint(len(cand))])
        taken[i] = True
        return i

    if empty_block is not None:
        assert 0 <= empty_block and empty_block + 64 <= N
        y[empty_block:empty_block + 64] = MISSING
        taken[empty_block:empty_block + 64] = True
        out["empty_block"] = int(empty_block)
    if empty_person:
        i = pick_person(np.ones(N, dtype=bool))
        y[i] = MISSING
        out["empty_person"] = i
    if complete_case:
        i = pick_person(np.ones(N, dtype=bool))
        y[i] = _responses(rng, 1, J)[0]
        out["complete_case"] = i
    obs = y != MISSING
    if unanswered_item:
        cand = np.flatnonzero(obs.sum(0) > 0)
        j = int(cand[rng.randint(len(cand))])
        y[:, j] = MISSING
        obs[:, j] = False
        out["unanswered_item"] = j
    seen = obs.sum(1) > 0
    j1 = j0 = None
    if constant_items:
        # two items with two respondents at least; where constant persons are asked for as well, a pair of items that leaves
        # somebody who did not see the all-zero item (to answer 1 throughout) and somebody who did not see the all-one item
        cand = np.flatnonzero(obs.sum(0) >= 2)
        cand = cand[rng.permutation(len(cand))]
        for t in range(len(cand) - 1):
            j1, j0 = int(cand[t]), int(cand[t + 1])
            if not constant_persons or ((seen & ~taken & ~obs[:, j0]).sum() >= 1 and (seen & ~taken & ~obs[:, j1]).sum() >= 2):
                break
        else:
            raise ValueError("no pair of items can be made constant beside the constant persons")
    i1 = i0 = None
    if constant_persons:
        i1 = pick_person(seen & (~obs[:, j0] if constant_items else True))
        i0 = pick_person(seen & (~obs[:, j1] if constant_items else True))
        y[i1, obs[i1]] = 1
        y[i0, obs[i0]] = 0
        out["all_one_person"], out["all_zero_person"] = i1, i0
    if constant_items:
        y[obs[:, j1], j1] = 1
        y[obs[:, j0], j0] = 0
        out["all_one_item"], out["all_zero_item"] = j1, j0
    d = describe(y)
    out.update({k: d[k] for k in ("missing", "n_missing", "min_obs", "max_obs", "empty_persons", "unanswered_items")})
    return y, out


def near_switch(N, J, frac, seed=0):
    """A design whose missing fraction is set EXACTLY: round(frac N J) cells are missing, counted, not drawn.  The cells go in a
    fixed order that depends on the seed alone (persons lose their cells at very different rates: at frac = 0.5 from a few per cent to all of them), so
    two calls with the same seed give the same persons and responses, the holes of the smaller frac inside those of the larger."""
    rng = np.random.RandomState(seed)
    y = _responses(rng, N, J)
    key = rng.rand(N, J) * np.logspace(-1.5, 0.0, N)[rng.permutation(N)][:, None]
    n_missing = int(round(frac * N * J))
    assert 0 <= n_missing <= N * J
    order = np.argsort(key, axis=None, kind="stable")
    y.reshape(-1)[order[:n_missing]] = MISSING
    d = describe(y)
    facts = {"design": "near_switch", "n_missing": n_missing, "missing": n_missing / float(N * J), "min_obs": d["min_obs"],
             "max_obs": d["max_obs"], "empty_persons": d["empty_persons"], "unanswered_items": d["unanswered_items"]}
    return y, facts


def all_missing(N, J):
    """No observed cell at all."""
    y = np.full((N, J), MISSING, dtype=np.uint8)
    return y, {"design": "all_missing", "n_missing": N * J, "missing": 1.0, "min_obs": 0, "max_obs": 0,
               "empty_persons": np.arange(N), "unanswered_items": np.arange(J)}


def single_cell(N, J, value=1):
    """One observed cell in the whole matrix (a person in the middle, an item a third of the way in)."""
    y = np.full((N, J), MISSING, dtype=np.uint8)
    i, j = N // 2, J // 3
    y[i, j] = value
    return y, {"design": "single_cell", "cell": (i, j), "n_missing": N * J - 1, "missing": (N * J - 1) / float(N * J),
               "min_obs": 0, "max_obs": 1, "empty_persons": np.delete(np.arange(N), i),
               "unanswered_items": np.delete(np.arange(J), j)}
