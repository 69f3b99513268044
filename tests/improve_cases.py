"""TEST INFRASTRUCTURE: inputs of the --improve-order tests, shared by the host and the GPU files.  A case is (ends int32 [n, 4], group int32 [n], n_groups,
order int32 [n], rev bool [n], start); the sequence is any valid one (the rule does not ask for the greedy order), so most cases start from a seeded shuffle
inside every group, which leaves the descent many rounds to take."""
import numpy as np

TOP = 1 << 30
BATCH = 32                       # IM_BATCH of csrc/gcode_improve.hip: rounds between two looks at the status word


def sequence(group, rng=None, reverse=False):
    """a valid drawing sequence: group after group, inside a group file order or a seeded shuffle; seeded directions when `reverse`"""
    group = np.asarray(group, np.int32)
    n = len(group)
    key = rng.permutation(n) if rng is not None else np.arange(n)
    order = key[np.argsort(group[key], kind="stable")].astype(np.int32)
    rev = rng.integers(0, 2, n).astype(bool) if (reverse and rng is not None) else np.zeros(n, bool)
    return order, rev


def random_plot(m, seed, n_groups=1, size=8000, longest=300, reverse=False, shuffle=True):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, size + 1, (m, 2))
    b = np.clip(a + rng.integers(-longest, longest + 1, (m, 2)), 0, size)
    group = rng.integers(0, n_groups, m).astype(np.int32)
    order, rev = sequence(group, rng if shuffle else None, reverse)
    return np.concatenate([a, b], 1).astype(np.int32), group, n_groups, order, rev, (0, 0)


def points(xs):
    """strokes of no length on the x axis, in file order, one group, from (0, 0)"""
    xs = np.asarray(xs, np.int64)
    e = np.stack([xs, np.zeros_like(xs), xs, np.zeros_like(xs)], 1).astype(np.int32)
    return e, np.zeros(len(xs), np.int32), 1, np.arange(len(xs), dtype=np.int32), np.zeros(len(xs), bool), (0, 0)


def strokes(rows):
    e = np.asarray(rows, np.int32).reshape(-1, 4)
    return e, np.zeros(len(e), np.int32), 1, np.arange(len(e), dtype=np.int32), np.zeros(len(e), bool), (0, 0)


# name -> (case, reverse, the move the first round must take: (code, i, second))
FIRST_MOVES = {
    "move_1_to_the_end": (points([10, 100, 20, 30]), False, (1, 1, 3)),
    "move_2_to_the_end": (points([10, 100, 110, 20, 30, 40]), False, (2, 1, 5)),
    "move_3_to_the_end": (points([10, 100, 110, 120, 20, 30, 40, 50]), False, (3, 1, 7)),
    "move_1_to_the_front": (points([50, 60, 5]), False, (1, 2, -1)),
    "move_2_to_the_front": (points([50, 60, 70, 5, 8]), False, (2, 3, -1)),
    "move_3_to_the_front": (points([50, 60, 70, 80, 5, 8, 11]), False, (3, 4, -1)),
    "reverse_the_open_end": (points([10, 40, 30, 20]), True, (0, 1, 3)),
    "flip_one_stroke": (strokes([[0, 0, 10, 0], [30, 0, 20, 0], [30, 0, 40, 0]]), True, (0, 1, 1)),
}


def tiny(m, reverse):
    """m = 0 .. 4 strokes, shuffled: blocks of three leave p almost no room"""
    return random_plot(m, 40 + m, size=50, longest=20, reverse=reverse)


def identical(m=9):
    e = np.tile(np.array([[7, 9, 7, 9]], np.int32), (m, 1))
    return e, np.zeros(m, np.int32), 1, np.arange(m, dtype=np.int32), np.zeros(m, bool), (3, 3)


def lattice(reverse, m=64, seed=5):
    """coordinates 0 .. 7: many equal gains, the tie-break decides"""
    return random_plot(m, seed, size=7, longest=7, reverse=reverse)


def corners(reverse, seed=6):
    """ends at 0 and 2^30 in both coordinates: sums of three distances leave int32"""
    rng = np.random.default_rng(seed)
    e = (rng.integers(0, 2, (12, 4)) * TOP).astype(np.int32)
    group = np.zeros(12, np.int32)
    order, rev = sequence(group, rng, reverse)
    return e, group, 1, order, rev, (TOP, 0)


def four_groups(reverse, seed=8):
    """groups 0 and 3 empty; group 2 sits 2^29 away from where group 1 ends, so its cursor arrives from there"""
    rng = np.random.default_rng(seed)
    e1 = rng.integers(0, 400, (14, 4)); e2 = rng.integers(0, 400, (11, 4)) + (1 << 29)
    e = np.concatenate([e1, e2]).astype(np.int32)
    group = np.concatenate([np.full(14, 1), np.full(11, 2)]).astype(np.int32)
    mix = rng.permutation(25)
    e, group = e[mix], group[mix]
    order, rev = sequence(group, rng, reverse)
    return e, group, 4, order, rev, (100, 100)


def tool_gcode(m=90, seed=12):
    """a seeded G-code text of m short strokes on an A4 sheet, in mm"""
    rng = np.random.default_rng(seed)
    lines = ["G21 G90 M5"]
    for _ in range(m):
        a = rng.uniform(5, 190, 2); b = np.clip(a + rng.uniform(-6, 6, 2), 1, 200)
        lines += ["G0 X%.2f Y%.2f" % tuple(a), "M3", "G1 X%.2f Y%.2f" % tuple(b), "M5"]
    return "\n".join(lines) + "\n"
