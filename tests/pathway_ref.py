"""The numpy restatement of the pathway maps (include/parasitoid_hip.h, ps_pathway_*), statement by statement: per
threshold the slots in ascending order, O_s = {v_s >= t}, the patches and labels of patch_ref.labels; every cell a
state 0 unreached, 1 front, 2 jump, 3 secondary; with the states as they stood before the slot a patch is `origin`
if it holds an anchor or a cell in state 1 and `seeded` if it holds a cell in a non-zero state; its cells still in
state 0 become 1 if origin, else 3 if seeded, else 2 (one focus founded); a state is never changed once set.
`classify` goes through patch_ref.labels; `flood_classify` is the same in plain Python over a flood fill, which the
CPU test pins it with.  `sequences(N)` are the crafted time sequences of fields with values in {0, 1, 2, 3} that the
CPU and the GPU tests share: with the thresholds patch_ref.SHAPE_THR one sequence gives three nested histories."""
import numpy as np

import patch_ref as P

CLASSES = ('front', 'jump', 'secondary')
ROW = ('front', 'jump', 'secondary', 'foci')
NSLOT = 4            # the slots of every crafted sequence
NEGVAL = 1e-8


def record_value(r, negval=NEGVAL):
    """what ps_record_value makes of a raw record with both scales 1 and no delta"""
    r = np.asarray(r, dtype=np.float64)
    return np.where((r != 0.0) & ~(r < negval), r, 0.0)


def classify(fields, threshold, connectivity, anchors, label_fn=P.labels):
    """one member, one threshold: fields [nslot, N, N] -> (state [N, N] int64, rows [nslot, 4] int64)"""
    fields = np.asarray(fields)
    nslot, N = fields.shape[0], fields.shape[1]
    state = np.zeros(N * N, dtype=np.int64)
    rows = np.zeros((nslot, 4), dtype=np.int64)
    for s in range(nslot):
        lab = label_fn(fields[s] >= threshold, connectivity).ravel()
        before = state.copy()                                  # the states as they stood before this slot
        cells = np.flatnonzero(lab >= 0)
        root = lab[cells]
        origin = np.zeros(N * N, dtype=bool)                   # per label
        seeded = np.zeros(N * N, dtype=bool)
        origin[root[before[cells] == 1]] = True
        for r, c in anchors:
            if lab[r * N + c] >= 0:
                origin[lab[r * N + c]] = True
        seeded[root[before[cells] != 0]] = True
        cls = np.where(origin[root], 1, np.where(seeded[root], 3, 2))
        new = before[cells] == 0
        state[cells[new]] = cls[new]
        for j in range(3):
            rows[s, j] = int((cls[new] == j + 1).sum())
        rows[s, 3] = int(np.unique(root[~origin[root] & ~seeded[root]]).size)
    return state.reshape(N, N), rows


def flood_classify(fields, threshold, connectivity, anchors):
    """the same in plain Python: the patches as lists of cells from patch_ref.flood_labels, one patch at a time"""
    fields = np.asarray(fields)
    nslot, N = fields.shape[0], fields.shape[1]
    state = [[0] * N for _ in range(N)]
    rows = [[0, 0, 0, 0] for _ in range(nslot)]
    anchors = set((int(r), int(c)) for r, c in anchors)
    for s in range(nslot):
        lab = P.flood_labels(fields[s] >= threshold, connectivity)
        patches = {}
        for r in range(N):
            for c in range(N):
                if lab[r, c] >= 0:
                    patches.setdefault(int(lab[r, c]), []).append((r, c))
        before = [row[:] for row in state]
        for q in sorted(patches):
            Q = patches[q]
            origin = any(cell in anchors or before[cell[0]][cell[1]] == 1 for cell in Q)
            seeded = any(before[r][c] != 0 for r, c in Q)
            cls = 1 if origin else (3 if seeded else 2)
            for r, c in Q:
                if before[r][c] == 0:
                    state[r][c] = cls
                    rows[s][cls - 1] += 1
            if cls == 2:
                rows[s][3] += 1
    return np.array(state, dtype=np.int64), np.array(rows, dtype=np.int64)


def accumulate(fields, weights, thresholds, connectivity, anchors, fn=classify):
    """fields: per member [nslot, N, N]; -> {'front', 'jump', 'secondary': [K, N, N] int64, 'rows': [members, K,
    nslot, 4] int64 (ROW)}"""
    fields = [np.asarray(f) for f in fields]
    nslot, N = fields[0].shape[0], fields[0].shape[1]
    K = len(thresholds)
    out = {name: np.zeros((K, N, N), dtype=np.int64) for name in CLASSES}
    out['rows'] = np.zeros((len(fields), K, nslot, 4), dtype=np.int64)
    for m, (F, w) in enumerate(zip(fields, weights)):
        for k, t in enumerate(thresholds):
            state, rows = fn(F, t, connectivity, anchors)
            for j, name in enumerate(CLASSES):
                out[name][k] += int(w) * (state == j + 1)
            out['rows'][m, k] = rows
    return out


def sequences(N):
    """[(name, [NSLOT, N, N] float64 with values in {0, 1, 2, 3}, anchors [(row, col), ...])], N odd and >= 17.
    The named history is the one at 0.5; the anchors are the centre cell unless the name says otherwise."""
    c = N // 2
    centre = [(c, c)]
    out = []

    def blank():
        return np.zeros((NSLOT, N, N))

    def origin(f, v=3.0):
        f[:, c - 1:c + 2, c - 1:c + 2] = v                    # the 3 x 3 origin patch, in every slot
        return f
    out.append(('empty', blank(), centre))
    f = blank()                                               # an anchor patch that only grows: all front
    for s in range(NSLOT):
        f[s, c - s - 2:c + s + 3, c - s - 2:c + s + 3] = 1.0
        f[s, c - s - 1:c + s + 2, c - s - 1:c + s + 2] = 2.0
        f[s, c - s:c + s + 1, c - s:c + s + 1] = 3.0
    out.append(('grow', f, centre))
    f = origin(blank())                                       # jump, secondary, merged: later cells front
    f[0:, c - 1:c + 2, c + 5:c + 7] = 2.0
    f[0:, c, c + 5] = 3.0                                     # at 2.5 one cell that never merges
    f[1:, c - 1:c + 2, c + 4:c + 8] = np.maximum(f[1:, c - 1:c + 2, c + 4:c + 8], 2.0)
    f[2:, c, c + 2:c + 4] = 2.0                               # the bridge
    f[3:, c - 2:c + 3, c + 8] = 1.0
    out.append(('jump_grow_merge', f, centre))
    f = origin(blank())                                       # two foci in one slot, one diagonal to the origin
    f[1:, c + 2:c + 4, c + 2:c + 4] = 3.0
    f[1:, c - 6:c - 4, c - 6:c - 4] = 2.0
    f[3, c + 4, c + 2:c + 4] = 1.0
    out.append(('two_foci_diagonal', f, centre))
    f = origin(blank())                                       # a focus drops out; its ground is re-entered
    f[0, c + 4:c + 6, c - 6:c - 3] = 3.0
    f[2, c + 5:c + 8, c - 4:c - 2] = 2.0                      # overlaps (c + 5, c - 4) of the old focus
    f[3, c + 5:c + 8, c - 4:c - 2] = 0.0
    f[3, 1:3, 1:3] = 1.0                                      # and a new focus elsewhere in the last slot
    out.append(('dropout_reenter', f, centre))
    f = blank()                                               # the anchor outside O in slot 0, inside it later
    f[:, 2:4, 2:5] = 2.0
    for s in range(1, NSLOT):
        f[s, c - s:c + s + 1, c - s:c + s + 1] = 3.0
    out.append(('anchor_late', f, centre))
    f = origin(blank())                                       # a patch holding state-1 and state-2 cells
    f[:, c - 1:c + 2, c + 4:c + 6] = 2.0
    f[1:, c, c + 2:c + 4] = 2.0                               # the bridge and, at once, more cells at the far end
    f[1:, c - 2:c + 3, c + 6] = 2.0
    f[2:, c + 3, c + 4:c + 7] = 3.0
    out.append(('origin_wins', f, centre))
    f = origin(blank())                                       # a second anchor makes the far blob front
    f[:, 2:5, 2:5] = 2.0
    f[1:, 2:5, N - 5:N - 2] = 2.0
    f[2:, 5, 2:5] = 3.0
    out.append(('two_anchors', f, centre + [(3, 3)]))
    f = blank()                                               # an island focus inside an origin ring
    f[:, c:c + 9, c:c + 9] = 2.0
    f[:, c + 1:c + 8, c + 1:c + 8] = 0.0                      # the ring, a corner on the anchor
    f[1:, c + 4, c + 4] = 3.0
    f[2:, c + 3:c + 6, c + 4] = 2.0
    f[3:, c + 1:c + 4, c + 4] = 1.0                           # it touches the ring at last
    out.append(('ring_island', f, centre))
    f = origin(blank())                                       # no wrap: (3, N - 1) and (4, 0) are two foci
    f[1:, 3, N - 1] = f[1:, 4, 0] = 3.0
    f[2:, 3, N - 2] = f[2:, 4, 1] = 2.0
    out.append(('edge_next_row', f, centre))
    f = origin(blank())                                       # the last cell alone as a focus
    f[2:, N - 1, N - 1] = 3.0
    out.append(('last', f, centre))
    return out
