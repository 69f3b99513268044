"""The sequence of stage-04 steps that tests/test_gpu_memo_reuse.py (device) and tests/test_memo_reuse_host.py (walker.h on the CPU) run over ONE memo
that is never cleared as a whole.  Maps come from the closed shapes of tests/contour_cases.py (no endpoint: every pixel is reached by leftover walks,
which fill the memo).  Plain numpy: nothing here touches the oracle or the device."""
import numpy as np

import contour_cases as C

H, W = 160, 200


def _stack(maps, h, w, at):
    out = np.zeros((len(maps), h, w), np.uint8)
    for k, m in enumerate(maps):
        C._put(out[k], m, *at)
    return out


def shapes():
    """K = 4: two figure eights, two rings joined by two bridges, a ring of 160 degree-2 pixels"""
    return [C.figure_eight(40, 70), C.nested(60, 80, 6, 2), C.diamond(C.RING_R, False), C.figure_eight(20, 30, True)]


_seq = []


def sequence():
    """[(tag, uint8 [K,H,W])], in the order the steps run; the same tag is the same array.
      A          the four shapes at (3, 3)
      A_shift    the same at (4, 4): its skeleton pixels lie next to and partly on A's, so stale words sit at and beside the live ones
      A_T        the shapes transposed, same image size
      A          again
      A_k2, A    the first two layers alone, then all four: planes 2 and 3 keep what the step before the last left
      B          H and W swapped (A's layers transposed as images): the old words land at other pixels
      A          again"""
    if not _seq:
        s = shapes()
        A = _stack(s, H, W, (3, 3))
        A_shift = _stack(s, H, W, (4, 4))
        A_T = _stack([m.T.copy() for m in s], H, W, (3, 3))
        B = np.ascontiguousarray(A.transpose(0, 2, 1))
        _seq.extend([("A", A), ("A_shift", A_shift), ("A_T", A_T), ("A", A), ("A_k2", A[:2].copy()), ("A", A), ("B", B), ("A", A)])
    return _seq
