"""TEST INFRASTRUCTURE: numpy stand-in for orip_stream_codes (the HIP kernel) so that the host logic of orip/stream.py can be checked on the CPU
against the reference's golden bytes.  Same closed form as csrc/stream.hip; itself pinned by the `bres*` golden vectors and, on segments of up to 200 000 steps, by the
digests of golden_stream_long.npz.  Also two independent checks
that once were the product's own code: a vectorised packer of a piece table (fill_bytes) and the corner flags of ONE polyline (corner_flags)."""
import math

import numpy as np


def codes_numpy(moves):
    m = np.asarray(moves, np.int64).reshape(-1, 4)
    dx, dy = np.abs(m[:, 2] - m[:, 0]), np.abs(m[:, 3] - m[:, 1])
    cnt = np.maximum(dx, dy)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    seg = np.repeat(np.arange(len(m)), cnt)
    k = np.arange(int(off[-1])) - off[seg]
    DX, DY = dx[seg], dy[seg]
    xpos, ypos = (m[:, 0] < m[:, 2])[seg], (m[:, 1] < m[:, 3])[seg]

    def cdiv0(a, b):
        return np.where(a <= 0, 0, -((-a) // np.maximum(b, 1)))
    xmaj = DX >= DY
    mx = np.where(xmaj, True, cdiv0(2 * (k + 1) * DX - DY, 2 * DY) != cdiv0(2 * k * DX - DY, 2 * DY))
    my = np.where(xmaj, cdiv0(2 * (k + 1) * DY - DX, 2 * DX) != cdiv0(2 * k * DY - DX, 2 * DX), True)
    diag = np.where(xpos, np.where(ypos, 1, 3), np.where(ypos, 7, 5))
    c = np.where(mx & my, diag, np.where(mx, np.where(xpos, 2, 6), np.where(ypos, 0, 4)))
    return off, c.astype(np.uint8)


def fill_bytes(T, codes):
    """The bytes of a piece table with numpy: index arrays per output byte, one code fetched per step.  orip_stream_pack does the same on
    the device; this is the fast packer next to gcode_double.pack_numpy, which goes piece by piece."""
    out = np.zeros(T.nbytes, np.uint8)
    out[T.svc_pos] = T.svc_val
    if len(T.pos):
        has = T.speed >= 0
        out[T.pos[has]] = T.speed[has].astype(np.uint8)
        pc = T.cnt.astype(np.int64)
        nb = (pc + 1) // 2                                                # step bytes per piece
        bpiece = np.repeat(np.arange(len(pc)), nb)
        j = np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)  # index of the byte inside its piece
        a = codes[T.code0[bpiece] + 2 * j].astype(np.int64) & 7
        has_b = 2 * j + 1 < pc[bpiece]
        b = np.where(has_b, codes[np.minimum(T.code0[bpiece] + 2 * j + 1, max(len(codes) - 1, 0))].astype(np.int64) & 7, 0)
        out[(T.pos + has)[bpiece] + j] = np.where(has_b, 0x80 | 0x40 | (a << 3) | b, 0x80 | (a << 3)).astype(np.uint8)
    return out.tobytes()


def _angle(a, b, c):                                                   # angle_degrees, helper :242-249 (Python floats, libm)
    v1x, v1y, v2x, v2y = a[0] - b[0], a[1] - b[1], c[0] - b[0], c[1] - b[1]
    n1, n2 = math.hypot(v1x, v1y), math.hypot(v2x, v2y)
    if n1 == 0 or n2 == 0:
        return 180.0
    return math.degrees(math.acos(max(-1.0, min(1.0, (v1x * v2x + v1y * v2y) / (n1 * n2)))))


def corner_flags(pl, corner_deg):
    """slow_in / slow_out of every segment of a polyline in step space (emit_polyline, helper :300-312).  The interior angle at vertex j is
    computed vectorised; a vertex whose angle comes out within 1e-6 degrees of the threshold is decided again with the helper's scalar
    formula (math.hypot / acos / degrees), so the comparison is the reference's own arithmetic wherever it could matter."""
    n = len(pl)
    sharp = np.zeros(n, bool)                                           # sharp[j]: angle at vertex j (between j-1, j, j+1) below the threshold
    if n >= 3:
        p = pl.astype(np.float64)
        v1, v2 = p[:-2] - p[1:-1], p[2:] - p[1:-1]
        n1, n2 = np.hypot(v1[:, 0], v1[:, 1]), np.hypot(v2[:, 0], v2[:, 1])
        ok = (n1 > 0) & (n2 > 0)
        cosv = np.clip((v1[:, 0] * v2[:, 0] + v1[:, 1] * v2[:, 1]) / np.where(ok, n1 * n2, 1.0), -1.0, 1.0)
        ang = np.where(ok, np.degrees(np.arccos(cosv)), 180.0)
        sharp[1:-1] = ang < corner_deg
        for j in np.nonzero(np.abs(ang - corner_deg) < 1e-6)[0]:
            sharp[j + 1] = _angle(pl[j], pl[j + 1], pl[j + 2]) < corner_deg
    slow_in = sharp[:-1].copy(); slow_in[0] = False                     # segment i = (i, i+1): entry corner at vertex i (i > 0)
    slow_out = sharp[1:].copy(); slow_out[-1] = False                   # exit corner at vertex i + 1 (when a vertex i + 2 exists)
    return slow_in, slow_out
