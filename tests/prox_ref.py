"""The numpy restatement of the proximity fields (include/parasitoid_hip.h, ps_prox_*) in integers: the distance
along every row to the nearest cell of the set, then the minimum over the rows of dy^2 + g^2, then
sqrt(d2.astype(float64)) * cell_m.  Also the crafted sets the CPU, GPU and host-emulation tests share."""
import numpy as np

NONE = 1 << 40          # "this row holds no cell of the set": larger than any squared distance


def far2(N):
    return 2 * (N - 1) ** 2 + 1


def reached(v, t, side='to'):
    """the set searched for: {v >= t}, or for 'in' its complement within the domain"""
    s = np.asarray(v) >= t
    return ~s if side == 'in' else s


def row_distance(s):
    """g[y, x] = min |x - x'| over the cells (y, x') of the set, NONE where row y holds none (int64)"""
    s = np.asarray(s, dtype=bool)
    N0, N1 = s.shape
    x = np.arange(N1, dtype=np.int64)
    left = np.maximum.accumulate(np.where(s, x, -NONE), axis=1)                        # the last set column <= x
    right = np.minimum.accumulate(np.where(s, x, NONE)[:, ::-1], axis=1)[:, ::-1]      # the first set column >= x
    return np.minimum(np.where(left < 0, NONE, x - left), np.where(right >= NONE, NONE, right - x))


def d2(s):
    """[N, N] uint32: the squared Euclidean distance in cells from every cell to the set, far2 where it is empty"""
    s = np.asarray(s, dtype=bool)
    N = s.shape[0]
    assert s.shape == (N, N)
    g = row_distance(s)
    g2 = np.where(g >= NONE, NONE, g * g)
    y = np.arange(N, dtype=np.int64)
    out = np.full((N, N), NONE, dtype=np.int64)
    for yy in range(N):                      # the row the nearest cell lies in
        np.minimum(out, ((y - yy) ** 2)[:, None] + g2[yy][None, :], out=out)
    out = np.where(out >= NONE, far2(N), out)
    return out.astype(np.uint32)


def metres(d2_plane, cell_m):
    """the field: fl(fl(sqrt((double) d2)) * cell_m)"""
    return np.sqrt(d2_plane.astype(np.float64)) * np.float64(cell_m)


def field(v, t, side, cell_m):
    """(d2, metres) of one window over the member's field v"""
    plane = d2(reached(v, t, side))
    return plane, metres(plane, cell_m)


def crafted(N):
    """[(name, bool [N, N])]: single cells in the corners and at the centre, a full row and column, only column 63,
    64 or N - 1 (the edges of the mask words), two cells equidistant from a third, a checkerboard, a ring with a
    hole, the empty set and the whole domain"""
    out = []
    c = N // 2
    for k, (y, x) in enumerate([(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)]):
        s = np.zeros((N, N), dtype=bool)
        s[y, x] = True
        out.append(('corner%d' % k, s))
    s = np.zeros((N, N), dtype=bool)
    s[c, c] = True
    out.append(('centre', s))
    s = np.zeros((N, N), dtype=bool)
    s[c // 2, :] = True
    s[:, c + 3] = True
    out.append(('row_and_column', s))
    s = np.zeros((N, N), dtype=bool)
    s[c + 7, :] = True
    out.append(('row', s))
    s = np.zeros((N, N), dtype=bool)
    s[:, c // 2] = True
    out.append(('column', s))
    for col in (63, 64, N - 1):
        s = np.zeros((N, N), dtype=bool)
        s[:, col] = True
        out.append(('column%d' % col, s))
    s = np.zeros((N, N), dtype=bool)
    s[c, c - 5] = s[c, c + 5] = True        # (c, c) and the whole column c are equidistant from both
    out.append(('equidistant', s))
    yy, xx = np.mgrid[:N, :N]
    out.append(('checkerboard', ((yy + xx) & 1).astype(bool)))
    r2 = (yy - c) ** 2 + (xx - c) ** 2
    out.append(('ring', (r2 >= (N // 8) ** 2) & (r2 <= (N // 3) ** 2)))
    out.append(('empty', np.zeros((N, N), dtype=bool)))
    out.append(('whole', np.ones((N, N), dtype=bool)))
    return out


def as_field(s, t):
    """a field whose set at threshold t is s: exactly t on the set (in it), one ulp below t elsewhere (not in it)"""
    return np.where(s, np.float64(t), np.nextafter(np.float64(t), 0.0))
