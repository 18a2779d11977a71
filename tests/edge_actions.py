"""Edge-action table and schedules shared by the fixture generator and the step tests.

The step kernels decide on `norm > 1`, `total > 0`, `x / norm` and the clips; the rows below sit on those decisions
(all float32, U = nextafter(1, 2)):
  nonfinite       norm inf, x / inf: NaN for the infinite component, 0 for a finite one
  overflow        finite components whose squared norm overflows float32: norm inf, the move is [0, 0]
  below_overflow  squared norm just below float32's maximum
  norm1           norm exactly 1 (not projected), one ulp above it (projected), 0.6^2 + 0.8^2 rounded
  zero            [0, 0] and [-0, 0]
  tiny            moves that vanish in the square, in the norm, or when added to a position
A schedule alternates ordinary uniform actions (even steps) with table rows (odd steps) so envs keep moving.
"""

import numpy as np

U = np.nextafter(np.float32(1), np.float32(2))
INF = np.float32(np.inf)
EDGE_CLASSES = {
    "nonfinite": [[INF, 0], [0, -INF], [INF, INF]],
    "overflow": [[3e19, 1], [-3e19, -3e19], [2e19, 2e19]],
    "below_overflow": [[1.8e19, 0.3]],
    "norm1": [[1, 0], [U, 0], [0.6, 0.8], [-1, 0], [0, -U]],
    "zero": [[0, 0], [-0.0, 0.0]],
    "tiny": [[1e-45, 0], [1e-30, 1e-30], [2**-20, 0], [0, -(2**-22)], [3e-8, 3e-8], [1e-8, 0]],
}
CLASS_NAMES = list(EDGE_CLASSES)
_ROWS = np.array([r for rows in EDGE_CLASSES.values() for r in rows], np.float32)
_ROW_CLASS = np.array([c for c, rows in enumerate(EDGE_CLASSES.values()) for _ in rows])
NONFINITE = CLASS_NAMES.index("nonfinite")


def edge_schedule(steps, n, seed, scale=1.0, nonfinite=12):
    """float32 [steps, n, 2]: uniform(-scale, scale) on even steps; on odd steps every env gets a row of a finite
    class (class uniform, then row uniform).  `nonfinite` slots of the odd steps, drawn without replacement, get a
    non-finite row instead: few, because LightDark keeps a NaN position until the time limit."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-scale, scale, (steps, n, 2)).astype(np.float32)
    odd = np.arange(1, steps, 2)
    finite = [c for c in range(len(CLASS_NAMES)) if c != NONFINITE]
    cls = np.array(finite)[rng.integers(0, len(finite), (len(odd), n))]
    u = rng.random((len(odd), n))
    first = np.array([np.nonzero(_ROW_CLASS == c)[0][0] for c in range(len(CLASS_NAMES))])
    count = np.bincount(_ROW_CLASS)
    a[odd] = _ROWS[first[cls] + (u * count[cls]).astype(np.int64)]
    if nonfinite:
        slots = rng.choice(len(odd) * n, nonfinite, replace=False)
        rows = np.nonzero(_ROW_CLASS == NONFINITE)[0]
        a[odd[slots // n], slots % n] = _ROWS[rows[rng.integers(0, len(rows), nonfinite)]]
    return a


def edge_class_of(actions):
    """int [...]: the class index of each action that is, bit for bit, a table row; -1 for any other."""
    bits = np.ascontiguousarray(actions, np.float32).view(np.uint32)
    out = np.full(bits.shape[:-1], -1)
    for row, c in zip(_ROWS.view(np.uint32), _ROW_CLASS):
        out[(bits == row).all(-1)] = c
    return out


def edge_class_counts(actions, stepped=None):
    """{class name: hits}, counting only env-steps where `stepped` (bool, default all) is set: an env that
    autoresets on a step ignores its action."""
    cls = edge_class_of(actions)
    if stepped is not None:
        cls = np.where(stepped, cls, -1)
    return {name: int((cls == c).sum()) for c, name in enumerate(CLASS_NAMES)}


def assert_edges_hit(actions, stepped=None, nonfinite=True, at_least=10):
    counts = edge_class_counts(actions, stepped)
    for name, k in counts.items():
        if name == "nonfinite" and not nonfinite:
            assert k == 0, counts
        else:
            assert k >= at_least, counts
    return counts


def nonfinite_followups(actions, stepped, terminated, more=5):
    """Number of envs in which some non-finite action was stepped and the same episode went on for at least
    `more` further steps (no termination on the non-finite step or the `more - 1` after it)."""
    cls = edge_class_of(actions)
    steps, n = cls.shape
    envs = set()
    for t, i in zip(*np.nonzero((cls == NONFINITE) & stepped)):
        if t + more < steps and not terminated[t:t + more, i].any() and stepped[t:t + more + 1, i].all():
            envs.add(int(i))
    return len(envs)
