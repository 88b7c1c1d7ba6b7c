"""The numpy restatement of the patch maps (include/parasitoid_hip.h, ps_patch_*), statement by statement:
O = {v >= t}; a patch is a connected component of O under 4- or 8-connectivity without wrap; its label the smallest
linear index row * N + col of its cells; the main patch the one with the most cells, among equals the smallest
label; per member the row (npatch, cells, main_cells, main_label, sat_cells_max) and the planes main += w in the
main patch, sat += w in the rest of O.  `labels` goes through scipy.ndimage.label; `flood_labels` is a flood fill
in plain Python that the CPU test pins it with.  `shapes(N)` are the crafted fields with values in {0, 1, 2, 3}
that the CPU and the GPU tests share."""
import numpy as np

NONE = 0xffffffff
FIELDS = ('npatch', 'cells', 'main_cells', 'main_label', 'sat_cells_max')
SHAPE_THR = [0.5, 1.5, 2.5]


def labels(mask, connectivity):
    """[N, N] int64: per cell of `mask` the smallest linear index of its patch, -1 outside"""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    comp, n = ndimage.label(mask, structure=structure)
    out = np.full(mask.shape, -1, dtype=np.int64)
    if n:
        flat = comp.ravel()
        at = np.flatnonzero(flat)
        smallest = np.full(n + 1, mask.size, dtype=np.int64)
        np.minimum.at(smallest, flat[at], at)
        out.ravel()[at] = smallest[flat[at]]
    return out


def flood_labels(mask, connectivity):
    """the same by a flood fill in plain Python: cells in ascending order start a patch, which takes their index"""
    mask = np.asarray(mask, dtype=bool)
    nr, nc = mask.shape
    out = [[-1] * nc for _ in range(nr)]
    steps = [(dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr or dc) and (connectivity == 8 or not (dr and dc))]
    for r0 in range(nr):
        for c0 in range(nc):
            if mask[r0, c0] and out[r0][c0] < 0:
                out[r0][c0] = r0 * nc + c0
                stack = [(r0, c0)]
                while stack:
                    r, c = stack.pop()
                    for dr, dc in steps:
                        rr, cc = r + dr, c + dc
                        if 0 <= rr < nr and 0 <= cc < nc and mask[rr, cc] and out[rr][cc] < 0:
                            out[rr][cc] = r0 * nc + c0
                            stack.append((rr, cc))
    return np.array(out, dtype=np.int64)


def member(field, threshold, connectivity, label_fn=labels):
    """one member, one threshold, one slot -> (row dict of FIELDS, main mask, satellite mask)"""
    mask = np.asarray(field) >= threshold
    lab = label_fn(mask, connectivity)
    roots, size = np.unique(lab[lab >= 0], return_counts=True)        # ascending labels
    row = dict(npatch=int(roots.size), cells=int(mask.sum()), main_cells=0, main_label=NONE, sat_cells_max=0)
    main = np.zeros(mask.shape, dtype=bool)
    if roots.size:
        i = int(np.argmax(size))                   # the first of the largest: the smallest label among equals
        row['main_cells'], row['main_label'] = int(size[i]), int(roots[i])
        others = np.delete(size, i)
        row['sat_cells_max'] = int(others.max()) if others.size else 0
        main = lab == roots[i]
    return row, main, mask & ~main


def accumulate(fields, weights, thresholds, connectivity, label_fn=labels):
    """fields: per member [nslot, N, N]; -> {'main', 'sat': [K, nslot, N, N] int64, FIELDS: [members, K, nslot] int64}"""
    fields = [np.asarray(f) for f in fields]
    nslot, N = fields[0].shape[0], fields[0].shape[1]
    K = len(thresholds)
    out = {'main': np.zeros((K, nslot, N, N), dtype=np.int64), 'sat': np.zeros((K, nslot, N, N), dtype=np.int64)}
    for name in FIELDS:
        out[name] = np.zeros((len(fields), K, nslot), dtype=np.int64)
    for m, (F, w) in enumerate(zip(fields, weights)):
        for k, t in enumerate(thresholds):
            for s in range(nslot):
                row, main, sat = member(F[s], t, connectivity, label_fn)
                out['main'][k, s] += int(w) * main
                out['sat'][k, s] += int(w) * sat
                for name in FIELDS:
                    out[name][m, k, s] = row[name]
    return out


def spiral(N):
    """a one-cell-wide spiral from (0, 0) inwards: advance while the cell after the next is free, else turn right"""
    m = np.zeros((N, N), dtype=bool)
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    r = c = d = turned = 0
    m[0, 0] = True

    def inside(a, b):
        return 0 <= a < N and 0 <= b < N
    while turned < 2:
        dr, dc = step[d]
        nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if inside(nr, nc) and not m[nr, nc] and not (inside(fr, fc) and m[fr, fc]):
            r, c, turned = nr, nc, 0
            m[r, c] = True
        else:
            d, turned = (d + 1) % 4, turned + 1
    return m


def shapes(N):
    """[(name, [N, N] float64 with values in {0, 1, 2, 3})], N >= 12: with the thresholds SHAPE_THR one field gives
    three nested sets.  The named shape is the set at 0.5; most carry a smaller copy of a different kind above it."""
    out = []

    def blank():
        return np.zeros((N, N))
    out.append(('empty', blank()))
    f = np.ones((N, N))
    f[1:-1, 1:-1] = 2.0
    f[3::4, 3::4] = 3.0                                  # at 2.5 isolated cells, at 1.5 the interior
    out.append(('full', f))
    f = blank()
    f[0, 0] = 3.0
    out.append(('first', f))
    f = blank()
    f[-1, -1] = 3.0
    out.append(('last', f))
    rr, cc = np.indices((N, N))
    f = ((rr + cc) % 2 == 0) * 1.0
    f[(rr % 4 == 0) & (cc % 4 == 0)] = 3.0
    out.append(('checkerboard', f))
    sp = spiral(N)
    f = sp * 1.0
    f[sp & (rr >= N // 2)] = 2.0                          # the lower half of every arm: many arcs
    out.append(('spiral', f))
    f = blank()
    f[:-1, ::2] = 1.0
    f[-1, :] = 2.0                                        # teeth one cell apart that join only in the last row
    f[: N // 2, ::4] = 3.0
    out.append(('comb', f))
    for name, (c_up, c_down) in (('equal_left_first', (1, 8)), ('equal_right_first', (8, 1))):
        f = blank()
        f[1:3, c_up:c_up + 3] = 3.0
        f[5:7, c_down:c_down + 3] = 3.0
        f[9, 1:4] = 2.0                                   # a smaller third patch
        out.append((name, f))
    f = blank()
    f[2:4, 2:4] = 3.0
    f[4:6, 4:6] = 2.0
    out.append(('diagonal', f))
    f = blank()
    f[2:4, 6:8] = 2.0
    f[4:6, 4:6] = 3.0
    out.append(('antidiagonal', f))
    f = blank()
    f[2:9, 2:9] = 1.0
    f[3:8, 3:8] = 0.0
    f[5, 5] = 3.0
    out.append(('ring_island', f))
    f = blank()
    f[3, N - 1] = f[4, 0] = 3.0
    out.append(('edge_next_row', f))
    f = blank()
    f[3, N - 1] = f[5, 0] = 3.0
    out.append(('edge_two_rows', f))
    f = blank()
    f[-1, :] = 2.0
    f[:, -1] = 2.0
    f[0, 0] = 3.0
    out.append(('last_row_col', f))
    return out
