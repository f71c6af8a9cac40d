"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Nothing under tc_gan_amd/ imports this module.

The cases, inputs, fp64 results, error measures and tolerances that hold the feed-forward kernels (tc_gan_amd/csrc/ssn_ff.hip:
dense and connection-list forward, dense and connection-list second pass) to a plain numpy fp64 restatement ELEMENT BY ELEMENT
at every grid and list edge (tests/test_ff_edges_gpu.py), and that tests/test_ff_cases.py checks without a GPU.

Why its own inputs.  With the model script's inputs (RF_l = 2, RF_d = 0.3, stimuli {-1, 0, 1}^3) every receptive field spans the
whole box: the last grid point holds 4.3e-4 (box 12) or 1.2e-5 (box 40) of a stimulus's denominator, less than the tolerances
of tests/test_ff_gpu.py, the threshold exponent is always 1 and the backward is seen as five totals
(tests/test_ff_cases.py::test_the_gap_* records that).  Here, by construction and asserted by `conditions`:

  * receptive fields are narrow: sig = RF_w RF_d + RF_l lies in [0.6, 0.9] grid steps;
  * every stimulus sits next to a NAMED grid point, displaced by 0.32 ... 0.42 of a step on each axis (so the point's d^2 is
    not 0 and it counts in dsig too): the named point holds at least SHARE_MIN of its stimulus's denominator, and -- where
    the list is long enough to connect every named point in every unit -- of the absolute-term sum of the drive and of one
    dsig element (the backward runs one gq pattern per group of nsam x nhid stimuli: in pattern r the element (s, h) has ONE
    main stimulus, the others enter at a hundredth);
  * named points come from the kernels' index arithmetic (`named_points`): g = 0 and G - 1, the first point of the last
    16-byte group, both sides of the first sweep boundary (g = 1023 | 1024 with 16-byte loads, 255 | 256 with scalar ones), the
    first point of a ragged last sweep (its last point is G - 1), both sides of a z-row crossing inside a 16-byte group, for
    the connection-list lattice kernel the first point a ring refill loads and points with iz & 3 = 1, 2, 3, and for the two
    lattice kernels the first point of a (thread, sweep) whose incremental (bx, by, bz) advance carried in bz only, in by
    only, and in both (`advance_trace` is a plain restatement of that advance).  A 16-byte group never crosses an xy plane:
    G % 4 == 0 with box % 4 != 0 means box = 2 mod 4, and then box^2 is a multiple of 4 (`group_crossings` finds none;
    asserted for every box up to 64);
  * the lattice kernels take any 3 x 3 x 3 product lattice in the script's order, so the named points of a box are split
    into groups with at most three distinct indices per axis and each group is one case whose 27 products land on them;
  * TH_sam holds 0, +-1, +-1e-6 and negative values; strengths and the other threshold samples are redrawn until no output
    has |q - thr| within MARGIN x max(S, |thr|) (S below) of the kink, so the device's `out > 0` pattern is the oracle's.

The dense inputs are the scatter of the lists: FF_con = 1 at a unit's list entries and 0 elsewhere, FF_str the list's strength
there and a non-zero draw elsewhere (so FF_con is seen to multiply).

Measures, each on the element's own scale.  den: relative.  q: |delta| / S with S = sum_g e |w_g| / den.  out = relu(q - thr): the
same, after the part of |delta| that the rounding of thr itself explains is taken off -- `thr_tol` per (sample, unit):
TOLERANCE_MULTIPLE x the float32 oracle's deviation of thr plus the derived term below, plus u |out| for the subtraction; an
absolute error of thr has no place on the scale of a drive that may be far smaller than thr.  A term whose e lies below float32's
smallest normal number is held absolutely (it enters S as 2^-102 |w| = 2^-126 |w| / u).  Where a unit has no connection S = 0:
q must be exactly 0 and out exactly within `thr_tol` of relu(-thr).  dsig: |delta| / sum |terms|, the terms being
the products the sums run over with (w_g - q) written as two terms, as the connection-list kernel adds them:
sum_i |gq / den| sum_g e d^2 / sig^3 (|w_g| + |q|) (and the same weighted by RF_w).

Tolerance, per case and quantity: TOLERANCE_MULTIPLE x the deviation of this same oracle run in float32 (numpy; positions
formed as -3 + step ix in float32 as the kernels do), plus one derived term for what float32 numpy does not model.  With
u = 2^-24 and x = d^2 / (2 sig^2) the exponent argument of a term, a term's e carries at most
    D(x) = u (8 + 8 x):
8 u for the exponentials -- v_exp_f32 is 1 ulp = 2 u, the lattice kernels multiply three of them (6 u) with two roundings
(2 u) -- and 8 u x for the argument, whose absolute error passes into e one to one: v_rcp_f32 of sig^2 1 ulp (2 u), and six
roundings of u each (sig sig, the three squares and two additions of d^2 count 3 u on a sum of positive terms, the product with
1 / (2 sig^2), the log2(e) factor of __expf or of the lattice kernels' constant).  The derived term of a sum is D weighted
over its terms: den sum_g e D / sum_g e;  q that of sum e |w| plus that of den;  dsig sum |term| (D + 12 u) / sum |term|
(v_rcp_f32 of sig^3 2 u, sig^3 2 u, d^2 3 u, gq / den 1 u, four products 4 u).  The threshold's derived term (in `thr_tol`):
u (|thr| + |TH_sam|^a TH_d (3 + 3 ln 2 a |log2 |TH_sam||)) for __powf = exp2(a log2 .) with v_log_f32 and v_exp_f32 at 1 ulp
and the rounding of the product.  Nothing is fitted to a kernel; no tolerance may exceed
TOLERANCE_CAP (above it the inputs are at fault, not the bound).
"""
import collections
import math

import numpy as np

U = 2.0 ** -24
MARGIN = 1e-3                 # no |q - thr| within MARGIN x max(S, |thr|) of the kink
SHARE_MIN = 0.05
TOLERANCE_MULTIPLE = 4.0
TOLERANCE_CAP = 1e-4
SENSITIVITY = 10.0            # every defect of tests/test_ff_cases.py moves a checked element by this many tolerances
FF_MAX_NI = 32
SPECIAL_TH = (0.0, 1.0, -1.0, 1e-6, -1e-6, -0.5)

STIM_KINDS = ('free', 'lattice', 'lattice-ulp', 'lattice-perm')
ENTRIES = ('forward', 'forward_sparse', 'backward', 'backward_sparse')
Case = collections.namedtuple('Case', 'entry path box nsam nhid ni a ncon stim group')


# ------------------------------------------------------------------ the kernels' index arithmetic, restated
def advance_trace(box, pts):
    """The incremental advance of the two lattice kernels (`bz += sz; if (bz >= box) { bz -= box; ++by; } by += sy; ...`),
    restated: [(thread, sweep, g, (bx, by, bz), carried in bz, carried in by)] for every (thread, sweep) the loop visits, the
    two flags those of the advance that led there (None in sweep 0).  `pts` grid points per lane and sweep (4 or 1)."""
    G = box ** 3
    nv, stride = G // pts, 256 * pts
    sx, sy, sz = stride // (box * box), (stride % (box * box)) // box, stride % box
    out = []
    for t in range(min(256, nv)):
        g = t * pts
        bz, by, bx = g % box, (g // box) % box, g // (box * box)
        cz = cy = None
        for k, v in enumerate(range(t, nv, 256)):
            out.append((t, k, v * pts, (bx, by, bz), cz, cy))
            bz += sz
            cz = bz >= box
            if cz:
                bz -= box
                by += 1
            by += sy
            cy = by >= box
            if cy:
                by -= box
                bx += 1
            bx += sx
    return out


def carry_points(box, pts):
    """{'z' | 'y' | 'zy': g}: the first point of the first (thread, sweep) whose advance carried in bz only / by only / both."""
    found = {}
    for t, k, g, _, cz, cy in advance_trace(box, pts):
        if cz is None:
            continue
        kind = {(True, False): 'z', (False, True): 'y', (True, True): 'zy'}.get((cz, cy))
        if kind and kind not in found:
            found[kind] = g
    return found


def group_crossings(box):
    """(row, plane): the first 16-byte group (four consecutive g, G % 4 == 0) that holds points of two z rows of one xy plane,
    and the first that holds points of two xy planes, each as (last point before, first point after) or None."""
    G = box ** 3
    row = plane = None
    if G % 4:
        return row, plane
    for g0 in range(0, G, 4):
        if g0 // (box * box) != (g0 + 3) // (box * box):
            plane = plane or (((g0 + 3) // (box * box)) * box * box - 1, ((g0 + 3) // (box * box)) * box * box)
        elif g0 // box != (g0 + 3) // box and row is None:
            row = (((g0 + 3) // box) * box - 1, ((g0 + 3) // box) * box)
    return row, plane


def named_points(box, lattice):
    """{name: g}, in the order of their priority (a case with fewer stimuli than points takes the first ones)."""
    G = box ** 3
    pts = collections.OrderedDict()

    def add(name, g):
        if 0 <= g < G and g not in pts.values():
            pts[name] = g
    add('last', G - 1)
    add('first', 0)
    for width in ((4, 1) if G % 4 == 0 else (1,)):          # the backward and the generic list kernels always load scalars
        tag, sweep = ('vec' if width == 4 else 'scalar'), 256 * width
        if width == 4:
            add('last-group', 4 * ((G - 1) // 4))
        if G > sweep:
            add(tag + '-sweep0-end', sweep - 1)
            add(tag + '-sweep1-start', sweep)
            if G % sweep:
                add(tag + '-ragged-sweep-start', sweep * ((G - 1) // sweep))
    row, plane = group_crossings(box)
    assert plane is None
    if row:
        add('row-crossing-before', row[0])
        add('row-crossing-after', row[1])
    if lattice:
        if box % 4 == 0:                                     # the connection-list lattice kernel
            nv = G // 4
            g0 = 4 * 768 if nv > 768 else 4 * (nv // 2)
            if nv > 768:
                add('ring-refill', g0)
            for k in (1, 2, 3):
                add('iz&3=%d' % k, g0 + k)
        for kind, g in sorted(carry_points(box, 4 if G % 4 == 0 else 1).items()):
            add('carry-' + kind, g)
    return pts


def coords(box, g):
    return g // (box * box), (g // box) % box, g % box


def lattice_groups(box):
    """The named points of a box (lattice kernels included) in groups with at most three distinct indices per axis."""
    groups = []
    for name, g in named_points(box, True).items():
        c = coords(box, g)
        for grp in groups:
            if all(len(set(coords(box, q)[ax] for q in grp.values()) | {c[ax]}) <= 3 for ax in range(3)):
                grp[name] = g
                break
        else:
            groups.append(collections.OrderedDict([(name, g)]))
    return groups


def is_lattice(stim):
    """ssn_capi.hip `ff_lattice`: 27 stimuli that are a product lattice in the script's order, compared as float32."""
    s = np.asarray(stim, dtype='float32')
    if s.shape != (27, 3):
        return False
    i = np.arange(27)
    return bool((s[:, 0] == s[9 * (i // 9), 0]).all() and (s[:, 1] == s[3 * ((i // 3) % 3), 1]).all() and (s[:, 2] == s[i % 3, 2]).all())


def predicted_path(entry, box, stim, rf_w_aligned=True):
    """The launchers' rules (ssn_ff.hip `launch_ff_*`)."""
    lat = is_lattice(stim)
    if entry == 'forward':
        return 'lattice' if lat else 'generic'
    if entry == 'forward_sparse':
        return 'sparse-lattice' if lat and box % 4 == 0 and box ** 3 % 4 == 0 and rf_w_aligned else 'sparse-generic'
    return {'backward': 'generic', 'backward_sparse': 'sparse-generic'}[entry]


# ------------------------------------------------------------------ the cases
BOXES = (1, 2, 3, 5, 7, 13, 6, 10, 14, 4, 8, 12, 16, 20, 24, 40)
_A = (0.5, 1.0, 2.5)


def _make_cases():
    cases = []

    def both(entries, box, nsam, nhid, ni, a, ncon, stim, group=0):
        for e in entries:
            path = {'forward': 'lattice' if stim == 'lattice' else 'generic',
                    'forward_sparse': 'sparse-lattice' if stim == 'lattice' and box % 4 == 0 else 'sparse-generic',
                    'backward': 'generic', 'backward_sparse': 'sparse-generic'}[e]
            cases.append(Case(e, path, box, nsam, nhid, ni, a, ncon, stim, group))
    for k, box in enumerate(BOXES):
        G = box ** 3
        nhid = (1, 3)[k % 2]
        nsam = 3 if nhid == 1 else 2
        # every named point of the scalar and 16-byte sweeps next to a stimulus of its own (ni = 32 = FF_MAX_NI holds them all)
        both(ENTRIES, box, nsam, nhid, 32, _A[k % 3], min(G, 40), 'free')
        for grp in range(len(lattice_groups(box))):
            both(ENTRIES[:2], box, 2, (3, 1)[(k + grp) % 2], 27, _A[(k + grp + 1) % 3], min(G, 40), 'lattice', grp)
    # stimulus counts, 27 stimuli that must NOT take a lattice kernel, list lengths (box 12: two 16-byte sweeps, seven scalar)
    for j, ni in enumerate((1, 20, 26, 28)):
        both(ENTRIES, 12, 2, (1, 3)[j % 2], ni, _A[j % 3], 40, 'free')
    for stim in ('lattice-ulp', 'lattice-perm'):
        both(ENTRIES, 12, 2, 1, 27, 2.5, 40, stim)
        both(ENTRIES[:2], 40, 2, 1, 27, 0.5, 40, stim)
    both(ENTRIES[2:], 12, 2, 3, 27, 0.5, 40, 'lattice')       # the second passes have no lattice form: the same kernels
    for j, ncon in enumerate((255, 256, 257, 600)):
        both(ENTRIES, 12 if ncon < 600 else 16, 2, (3, 1)[j % 2], 20, _A[j % 3], ncon, 'free')     # (600 of 1728 would crowd a stimulus's neighbourhood)
    # box^3 / 100 = 0 is the list length the script draws on a box below 5; 0 and 1 on small boxes, where no term of a drive
    # is so far from its stimulus that float32 loses it
    for j, ncon in enumerate((0, 1)):
        both(ENTRIES, 3, 2, (3, 1)[j], 20, _A[j], ncon, 'free')
        both(ENTRIES[:2], 4, 2, (1, 3)[j], 27, _A[j + 1], ncon, 'lattice')
    return cases


CASES = _make_cases()


def case_id(c):
    return '%s-%s-box%d-s%dh%d-ni%d-a%g-ncon%d-%s%d' % (c.entry, c.path, c.box, c.nsam, c.nhid, c.ni, c.a, c.ncon, c.stim, c.group)


def _key(c):
    return c._replace(entry=None, path=None)


def _f32(a):
    return np.asarray(a, dtype='float64').astype('float32').astype('float64')


def values(c):
    """(model parameters as `ff_model` takes them -- logs --, the float32 numbers the kernels get from them as fp64)."""
    h = 6.0 / (c.box - 1) if c.box > 1 else 1.0
    want = dict(RF_l=float(np.float32(0.6 * h)), RF_d=float(np.float32(0.3 * h)), TH_d=0.375, J=3.0, a=c.a)
    params = dict(RF_low=math.log(want['RF_l']), RF_del=math.log(want['RF_d']), THR_del=math.log(want['TH_d']),
                  Js=math.log(want['J']), As=math.log(want['a']), THR=0.5)
    val = dict(RF_l=np.exp(params['RF_low']), RF_d=np.exp(params['RF_del']), TH=params['THR'], TH_d=np.exp(params['THR_del']),
               J=np.exp(params['Js']), a=np.exp(params['As']))
    return params, {k: float(np.float32(v)) for k, v in val.items()}


def positions(box, dtype='float64'):
    """(G, 3), z fastest.  fp64: linspace(-3, 3, box)^3 as the model script; float32: -3 + step ix in float32 as the kernels."""
    i = np.arange(box)
    if dtype == 'float64':
        a = np.linspace(-3, 3, box)
    else:
        step = np.float32(6) / np.float32(box - 1) if box > 1 else np.float32(0)
        a = np.float32(-3) + step * i.astype('float32')
    X, Y, Z = np.meshgrid(a, a, a, indexing='ij')
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3)


def _stimuli(c, rs):
    """(stim (ni, 3) float32-representable, named {name: (g, stimulus index)}, the grid point next to every stimulus -- named first)."""
    box, G = c.box, c.box ** 3
    step = 6.0 / (box - 1) if box > 1 else 0.0
    h = step if box > 1 else 1.0

    def disp(n):
        return rs.uniform(0.32, 0.42, n) * rs.choice([-1.0, 1.0], n) * h
    if c.stim == 'free':
        pts = list(named_points(box, False).items())[:c.ni]
        taken = set(g for _, g in pts)
        others = [g for g in rs.permutation(G)[:c.ni + len(taken)] if g not in taken]
        gs = [g for _, g in pts] + [others[j % len(others)] if others else pts[0][1] for j in range(c.ni - len(pts))]
        stim = np.array([[-3 + step * q for q in coords(box, g)] for g in gs]) + np.stack([disp(3) for _ in gs])
        return _f32(stim), collections.OrderedDict((name, (g, i)) for i, (name, g) in enumerate(pts)), list(dict.fromkeys(gs))
    grp = lattice_groups(box)[c.group]
    axes = []
    for ax in range(3):
        ids = sorted(set(coords(box, g)[ax] for g in grp.values()))
        spare = [j for j in list(range(box // 2, box + 3)) + list(range(box // 2)) if j not in ids]
        axes.append(ids + spare[:3 - len(ids)])
    vals = [np.array([-3 + step * j for j in ids]) + disp(3) for ids in axes]
    stim = _f32([[vals[0][a], vals[1][b], vals[2][k]] for a in range(3) for b in range(3) for k in range(3)])
    named = collections.OrderedDict()
    for name, g in grp.items():
        a, b, k = (axes[ax].index(coords(box, g)[ax]) for ax in range(3))
        named[name] = (g, (a * 3 + b) * 3 + k)
    if c.stim == 'lattice-ulp':                 # one coordinate of one stimulus one float32 ulp away: no lattice any more
        s32 = stim.astype('float32')
        s32[13, 1] = np.nextafter(s32[13, 1], np.float32(10))
        stim = s32.astype('float64')
    elif c.stim == 'lattice-perm':
        perm = rs.permutation(27)
        stim = stim[perm]
        named = collections.OrderedDict((n, (g, int(np.where(perm == i)[0][0]))) for n, (g, i) in named.items())
    else:
        assert c.stim == 'lattice'
    anchors = [g for _, (g, _) in named.items()]
    for a in range(3):
        for b in range(3):
            for k in range(3):
                if max(axes[0][a], axes[1][b], axes[2][k]) < box:
                    anchors.append((axes[0][a] * box + axes[1][b]) * box + axes[2][k])
    return stim, named, list(dict.fromkeys(anchors))


def _lists(c, anchors, rs):
    """conn_idx (nsam, nhid, ncon) int32 with -1 slots mid-list and at the end, named points at slots 0, 255, 256 and the last
    filled one where the list reaches that far."""
    G = c.box ** 3
    idx = np.full((c.nsam, c.nhid, c.ncon), -1, dtype='int32')
    pts = [int(g) for g in anchors]
    for s in range(c.nsam):
        for h in range(c.nhid):
            n_end = (s + h) % 3 if c.ncon >= 4 else ((s + h) % 2 if c.ncon else 0)
            n_mid = 1 + (s + 2 * h) % 2 if c.ncon >= 8 else 0
            n = max(0, min(c.ncon - n_end - n_mid, G))
            n_mid = c.ncon - n_end - n
            take = pts[:n]
            rest = [g for g in rs.permutation(G)[:n + len(take)] if g not in set(take)][:n - len(take)]
            gs = list(rs.permutation(np.array(take + rest, dtype='int64')))
            slots = sorted(rs.choice([k for k in range(1, c.ncon - n_end - 1) if k not in (255, 256)], n_mid, replace=False)) if n_mid else []
            filled = [k for k in range(c.ncon - n_end) if k not in slots]
            assert len(filled) == len(gs)
            for j, t in enumerate([0, filled[-1] if filled else 0, 255, 256]):       # named points at the list's own edges
                if j < len(take) and t in filled:
                    a, b = gs.index(take[j]), filled.index(t)
                    gs[a], gs[b] = gs[b], gs[a]
            idx[s, h, filled] = gs
    return idx


_INPUTS = {}


def inputs(c):
    """Everything a case's entry points take (fp64 arrays that are exactly float32 numbers; cached for the last input set)."""
    key = _key(c)
    if key in _INPUTS:
        return _INPUTS[key]
    _INPUTS.clear()
    seed = (((c.box * 41 + c.ni) * 7 + c.nhid) * 1009 + c.ncon) * 97 + int(c.a * 10) * 5 + c.group * 11 + STIM_KINDS.index(c.stim)
    rs = np.random.RandomState(seed)
    G = c.box ** 3
    params, val = values(c)
    stim, named, anchors = _stimuli(c, rs)
    rf_w = rs.rand(c.nsam, G)
    rf_w[:, anchors] = rs.uniform(0.0, 0.15, (c.nsam, len(anchors)))    # narrow at the points next to a stimulus: more of dsig
    x = dict(params=params, val=val, stim=stim, named=named, anchors=anchors, RF_w=_f32(rf_w), idx=_lists(c, anchors, rs))
    x['fields'] = [_fields(c, x, s, 'float64') for s in range(c.nsam)]
    special = [SPECIAL_TH[(j + c.box + c.ni) % len(SPECIAL_TH)] for j in range(c.nsam * c.nhid)]
    for rounds in range(200):
        x['str'] = _f32(rs.uniform(0.5, 1.0, x['idx'].shape))
        ths = rs.uniform(-1, 1, (c.nsam, c.nhid))
        keep = np.arange(c.nsam * c.nhid).reshape(c.nsam, c.nhid) % 2 == 0          # every other one a special value
        x['TH_sam'] = _f32(np.where(keep, np.reshape(special, (c.nsam, c.nhid)), ths))
        o = _results(c, x, x['fields'], 'float64')
        if kink_distance(o) >= MARGIN:
            break
    else:
        raise AssertionError('no draw off the kink: ' + case_id(c))
    x['rounds'] = rounds
    # the dense streams: the scatter of the lists; FF_str non-zero where FF_con is 0
    x['FF_con'] = np.zeros((c.nsam, c.nhid, G))
    x['FF_str'] = _f32(rs.uniform(0.5, 1.0, (c.nsam, c.nhid, G)))
    s, h, k = np.nonzero(x['idx'] >= 0)
    x['FF_con'][s, h, x['idx'][s, h, k]] = 1.0
    x['FF_str'][s, h, x['idx'][s, h, k]] = x['str'][s, h, k]
    # upstream gradients of the drive: pattern r gives element (s, h) ONE main stimulus, the others a hundredth of it
    per = c.nsam * c.nhid
    R = -(-c.ni // per)
    gq = rs.uniform(0.005, 0.01, (R, c.nsam, c.ni, c.nhid)) * rs.choice([-1.0, 1.0], (R, c.nsam, c.ni, c.nhid))
    main = np.zeros((R, c.nsam, c.nhid), dtype=int)
    for r in range(R):
        for s in range(c.nsam):
            for h in range(c.nhid):
                i = main[r, s, h] = (r * per + s * c.nhid + h) % c.ni
                gq[r, s, i, h] = rs.uniform(0.5, 1.0) * rs.choice([-1.0, 1.0])
    x['gq'], x['main'] = _f32(gq), main
    _INPUTS[key] = x
    return x


# ------------------------------------------------------------------ the oracle (numpy; fp64, or float32 for the tolerance)
def _fields(c, x, s, dtype, pos=None, rf_w=None):
    """The per-point quantities of sample s: d2, xarg, e, k = e d^2 / sig^3 (ni, G) and rw (G,)."""
    dt = np.dtype(dtype)
    v = {k: dt.type(q) for k, q in x['val'].items()}
    pos = positions(c.box, dtype) if pos is None else pos
    stim = x['stim'].astype(dt)
    rw = (x['RF_w'][s] if rf_w is None else rf_w).astype(dt)
    d = pos[None, :, :] - stim[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    sig = rw * v['RF_d'] + v['RF_l']
    xarg = d2 / (dt.type(2) * sig * sig)
    e = np.exp(-xarg)
    return dict(d2=d2, xarg=xarg, e=e, k=e * d2 / (sig * sig * sig), rw=rw)


def thresholds(c, x, dtype='float64'):
    dt = np.dtype(dtype)
    v = {k: dt.type(q) for k, q in x['val'].items()}
    ts = x['TH_sam'].astype(dt)
    return v['TH'] + np.sign(ts) * np.abs(ts) ** v['a'] * v['TH_d']


def _results(c, x, fields, dtype, with_bounds=False):
    """den (nsam, ni), q, out, S (nsam, ni, nhid) and the sums of the second pass A, Aabs (nsam, ni, nhid, 2), B (nsam, ni, 2)
    (element 1 weighted by RF_w), from the lists."""
    dt = np.dtype(dtype)
    J = dt.type(x['val']['J'])
    sh = (c.nsam, c.ni, c.nhid)
    o = dict(den=np.zeros(sh[:2], dt), num=np.zeros(sh, dt), absnum=np.zeros(sh, dt), B=np.zeros(sh[:2] + (2,), dt),
             A=np.zeros(sh + (2,), dt), Aabs=np.zeros(sh + (2,), dt))
    if with_bounds:
        o.update(denD=np.zeros(sh[:2]), numD=np.zeros(sh), BD=np.zeros(sh[:2] + (2,)), AD=np.zeros(sh + (2,)))
    for s, F in enumerate(fields):
        kk = np.stack([F['k'], F['k'] * F['rw'][None, :]], axis=-1)                  # (ni, G, 2)
        o['den'][s] = F['e'].sum(axis=1)
        o['B'][s] = kk.sum(axis=1)
        if with_bounds:
            D = U * (8 + 8 * F['xarg'])
            o['denD'][s] = (F['e'] * D).sum(axis=1)
            o['BD'][s] = (kk * (D + 12 * U)[..., None]).sum(axis=1)
        for h in range(c.nhid):
            ok = x['idx'][s, h] >= 0
            g, w = x['idx'][s, h][ok], J * x['str'][s, h][ok].astype(dt)
            o['num'][s, :, h] = (F['e'][:, g] * w).sum(axis=1)
            o['absnum'][s, :, h] = (F['e'][:, g] * np.abs(w)).sum(axis=1)
            o['A'][s, :, h] = (kk[:, g] * w[None, :, None]).sum(axis=1)
            o['Aabs'][s, :, h] = (kk[:, g] * np.abs(w)[None, :, None]).sum(axis=1)
            if with_bounds:
                o['numD'][s, :, h] = (F['e'][:, g] * np.abs(w) * D[:, g]).sum(axis=1)
                o['AD'][s, :, h] = (kk[:, g] * (np.abs(w)[None, :] * (D[:, g] + 12 * U))[..., None]).sum(axis=1)
    o['thr'] = thresholds(c, x, dtype)
    o['q'] = o['num'] / o['den'][:, :, None]
    # (a term whose e is below float32's smallest normal number 2^-126 is held absolutely, not relatively: it counts as 2^-102 = 2^-126 / u)
    wsum = np.array([[J * np.where(x['idx'][s, h] >= 0, x['str'][s, h], 0).sum() for h in range(c.nhid)] for s in range(c.nsam)])
    o['S'] = (o['absnum'] + dt.type(2.0 ** -102) * wsum[:, None, :].astype(dt)) / o['den'][:, :, None]
    o['out'] = np.maximum(o['q'] - o['thr'][:, None, :], dt.type(0))
    return o


def kink_distance(o):
    """Smallest |q - thr| / max(S, |thr|) over the outputs."""
    thr = np.broadcast_to(np.abs(o['thr'])[:, None, :], o['q'].shape)
    scale = np.maximum(o['S'], thr)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(scale > 0, np.abs(o['q'] - o['thr'][:, None, :]) / scale, np.inf)     # (thr = 0 without drive: out = 0 either way)
    return float(r.min())


def second_pass(o, gq, q, den, dtype='float64', with_bounds=False):
    """dsig (R, nsam, nhid, 2) written out directly: sum_i gq / den (sum_g k w_g - q sum_g k), its absolute-term sum, and (fp64)
    the derived bound in the measure.  q, den are INPUTS of the second pass (nsam, ni, nhid), as the kernels get them."""
    dt = np.dtype(dtype)
    coef = (gq.astype(dt) / den.astype(dt)[None])[..., None]                        # (R, nsam, ni, nhid, 1)
    qq = q.astype(dt)[None, ..., None]
    dsig = (coef * (o['A'][None] - qq * o['B'][None, :, :, None, :])).sum(axis=2)
    if dtype != 'float64':
        return dsig
    scale = (np.abs(coef) * (o['Aabs'][None] + np.abs(qq) * o['B'][None, :, :, None, :])).sum(axis=2)
    res = dict(dsig=dsig, scale=scale, coef=coef)
    if with_bounds:
        with np.errstate(invalid='ignore'):
            res['bound'] = (np.abs(coef) * (o['AD'][None] + np.abs(qq) * o['BD'][None, :, :, None, :])).sum(axis=2) / scale
    return res


_ORACLE = {}


def oracle(c):
    """fp64 results of a case's input set (cached for the last one): den (nsam, ni), q, out, S (nsam, ni, nhid), thr,
    q32, den32 (the second pass's inputs: q and den rounded to float32, den broadcast over the units),
    dsig, scale (R, nsam, nhid, 2), tol = {'den', 'q', 'out', 'dsig'}, dev32 and derived likewise."""
    key = _key(c)
    if key in _ORACLE:
        return _ORACLE[key]
    _ORACLE.clear()
    x = inputs(c)
    o = _results(c, x, x['fields'], 'float64', with_bounds=True)
    o['q32'] = _f32(o['q'])
    o['den32'] = _f32(np.broadcast_to(o['den'][:, :, None], o['q'].shape))
    o.update(second_pass(o, x['gq'], o['q32'], o['den32'], with_bounds=True))
    # the same in float32
    o32 = _results(c, x, [_fields(c, x, s, 'float32') for s in range(c.nsam)], 'float32')
    ts = np.abs(x['TH_sam'])
    pw = np.where(ts > 0, ts ** x['val']['a'], 0.0) * x['val']['TH_d']
    lg = np.where(ts > 0, np.abs(np.log2(np.where(ts > 0, ts, 1.0))), 0.0)
    o['thr_tol'] = TOLERANCE_MULTIPLE * np.abs(o32['thr'] - o['thr']) + U * (np.abs(o['thr']) + pw * (3 + 3 * math.log(2) * x['val']['a'] * lg))
    d32 = second_pass(o32, x['gq'], o['q32'], o['den32'], 'float32')
    dev = {k: float(v.max()) for k, v in errors(o, dict(den=o32['den'], q=o32['q'], out=o32['out'], dsig=d32)).items()}
    # the derived term
    with np.errstate(divide='ignore', invalid='ignore'):
        den_b = o['denD'] / o['den']
        q_b = np.where(o['S'] > 0, o['numD'] / o['absnum'], 0.0) + den_b[:, :, None]
    derived = dict(den=float(den_b.max()), q=float(q_b.max()), out=float(q_b.max()), dsig=float(np.nan_to_num(o['bound']).max()))
    o['dev32'], o['derived'] = dev, derived
    o['tol'] = {k: TOLERANCE_MULTIPLE * dev[k] + derived[k] for k in dev}
    assert all(0 <= t <= TOLERANCE_CAP for t in o['tol'].values()) and o['tol']['den'] > 0, (case_id(c), o['tol'], dev)
    _ORACLE[key] = o
    return o


def errors(o, got):
    """{quantity: the error of every element in its own measure} for whichever of den, q, out, dsig `got` holds.  den may come
    per unit (nsam, ni, nhid) as the kernels store it.  Where S = 0 (a unit without connections) q must be 0 exactly (any
    other value measures inf) and out is measured against |thr|."""
    res = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        if 'den' in got:
            den = o['den'] if np.ndim(got['den']) == 2 else o['den'][:, :, None]
            res['den'] = np.abs(got['den'] - den) / den
        if 'q' in got:
            d = np.abs(got['q'] - o['q'])
            res['q'] = np.where(o['S'] > 0, d / o['S'], np.where(d == 0, 0.0, np.inf))
        if 'out' in got:
            d = np.maximum(np.abs(got['out'] - o['out']) - o['thr_tol'][:, None, :] - U * o['out'], 0.0)
            res['out'] = np.where(o['S'] > 0, d / o['S'], np.where(d == 0, 0.0, np.inf))
        if 'dsig' in got:
            d = np.abs(got['dsig'] - o['dsig'])
            res['dsig'] = np.where(o['scale'] > 0, d / o['scale'], np.where(d == 0, 0.0, np.inf))
    return {k: np.where(np.isnan(v), np.inf, v) for k, v in res.items()}


def param_grads(c, o, r=0):
    """The gradient of sum(gq_r out) w.r.t. the five trainable (log) parameters from the oracle's own q, den, and the absolute
    tolerance that follows from the element tolerances when the second pass runs on the KERNEL's q, den (ff_model.ff_backward):
    dsig's own, den's through gq / den, q's through -q sum_g k; the drive sum's through q; the two threshold sums are fp64
    sums of float32 numbers on the host (u of their absolute sum)."""
    x = inputs(c)
    v, gq, tol = x['val'], x['gq'][r] * (o['out'] > 0), o['tol']       # (ff_backward masks the upstream gradient by out > 0)
    den = o['den'][:, :, None]
    sp = second_pass(o, gq[None], o['q'], np.broadcast_to(den, o['q'].shape))
    d, scale = sp['dsig'][0], sp['scale'][0]
    via_q = (np.abs(gq / den)[..., None] * o['B'][:, :, None, :] * (tol['q'] * o['S'])[..., None]).sum(axis=1)
    t_d = ((tol['dsig'] + tol['den']) * scale + via_q).sum(axis=(0, 1))
    ts = x['TH_sam']
    pw = np.sign(ts) * np.abs(ts) ** v['a']
    want = dict(RF_low=d[..., 0].sum() * v['RF_l'], RF_del=d[..., 1].sum() * v['RF_d'], Js=(gq * o['q']).sum(),
                THR=-gq.sum(), THR_del=-(gq * pw[:, None, :]).sum() * v['TH_d'])
    atol = dict(RF_low=t_d[0] * v['RF_l'], RF_del=t_d[1] * v['RF_d'], Js=(np.abs(gq) * o['S']).sum() * tol['q'],
                THR=U * np.abs(gq).sum(), THR_del=U * (np.abs(gq) * np.abs(pw)[:, None, :]).sum() * v['TH_d'])
    return want, atol


# ------------------------------------------------------------------ the conditions of a case
def fully_connected(c):
    """Every named point is on every unit's list."""
    x = inputs(c)
    return all(g in x['idx'][s, h] for g, _ in x['named'].values() for s in range(c.nsam) for h in range(c.nhid))


def shares(c):
    """{name: (share of den, share of sum e |w|, largest share of a dsig element's absolute-term sum)} of the named points, each
    the smallest over the samples (and units); the last two None unless `fully_connected`."""
    x, o = inputs(c), oracle(c)
    J, full, res = x['val']['J'], fully_connected(c), {}
    for name, (g, i) in x['named'].items():
        den = min(x['fields'][s]['e'][i, g] / o['den'][s, i] for s in range(c.nsam))
        num = dsg = None
        if full:
            num, per = [], []
            for s in range(c.nsam):
                F = x['fields'][s]
                for h in range(c.nhid):
                    w = J * x['str'][s, h][list(x['idx'][s, h]).index(g)]
                    num.append(F['e'][i, g] * w / o['absnum'][s, i, h])
                    term = np.abs(o['coef'][:, s, i, h, 0]) * F['k'][i, g] * (w + abs(o['q32'][s, i, h]))
                    per.append((term / o['scale'][:, s, h, 0]).max())
            num, dsg = min(num), max(per)
        res[name] = (float(den), num, dsg)
    return res


def conditions(c):
    """Asserts the conditions of the module docstring; returns the figures."""
    x, o = inputs(c), oracle(c)
    for k in ('stim', 'RF_w', 'str', 'TH_sam', 'FF_str', 'gq'):
        assert np.array_equal(x[k], _f32(x[k])), k
    sig = x['RF_w'] * x['val']['RF_d'] + x['val']['RF_l']
    h = 6.0 / (c.box - 1) if c.box > 1 else 1.0
    assert 0.6 * h * (1 - 1e-6) <= sig.min() and sig.max() <= 0.9 * h * (1 + 1e-6)
    assert x['named'] and len(set(i for _, i in x['named'].values())) == len(x['named'])
    sh = shares(c)
    for name, (den, num, dsg) in sh.items():
        assert den >= SHARE_MIN, (case_id(c), name, den)
        assert num is None or (num >= SHARE_MIN and dsg >= SHARE_MIN), (case_id(c), name, num, dsg)
    kink = kink_distance(o)
    assert kink >= MARGIN
    assert predicted_path(c.entry, c.box, x['stim']) == c.path, case_id(c)
    # the exponent arguments that matter: terms holding at least 2^-24 of their den
    big = max(float(F['xarg'][F['e'] >= U * F['e'].sum(axis=1, keepdims=True)].max()) for F in x['fields'])
    return dict(shares=sh, kink=kink, rounds=x['rounds'], xarg=big, positive=float((o['out'] > 0).mean()))


# ------------------------------------------------------------------ defects, for the sensitivity of the check
DEFECTS = ('dropped', 'weight-from-next', 'coordinate-from-neighbour')


def defect(c, g, kind):
    """The oracle's results with ONE grid point wrong in every sample: left out; reading RF_w, FF_con, FF_str (its list entry)
    at g + 1 (g - 1 for the last point); or placed at its neighbour's coordinates.  Returns what `errors` takes: den, q, out of
    the forward, and dsig of the second pass on the unchanged q32, den32 (the second pass's inputs do not change)."""
    x, o = inputs(c), oracle(c)
    G = c.box ** 3
    nb = g + 1 if g + 1 < G else g - 1
    pos = positions(c.box)
    idx, strn, fields = x['idx'], x['str'], []
    if kind == 'weight-from-next':
        # the list form of "FF_con, FF_str read at the neighbour": g's entry leaves, and the neighbour's (if any) counts at g too
        idx, strn = idx.copy(), strn.copy()
        for s in range(c.nsam):
            for h in range(c.nhid):
                at, an = np.where(x['idx'][s, h] == g)[0], np.where(x['idx'][s, h] == nb)[0]
                if len(at) and len(an):
                    strn[s, h, at[0]] = x['str'][s, h, an[0]]
                elif len(at):
                    idx[s, h, at[0]] = -1
    for s in range(c.nsam):
        F = dict(x['fields'][s])
        p, rw = pos[g:g + 1], x['RF_w'][s, g:g + 1]
        if kind == 'coordinate-from-neighbour':
            p = pos[nb:nb + 1]
        elif kind == 'weight-from-next':
            rw = x['RF_w'][s, nb:nb + 1]
        one = _fields(c, x, s, 'float64', pos=p, rf_w=rw)
        for k in ('xarg', 'e', 'k'):
            F[k] = F[k].copy()
            F[k][:, g] = 0.0 if kind == 'dropped' and k != 'xarg' else one[k][:, 0]
        if kind == 'weight-from-next':
            F['rw'] = F['rw'].copy()
            F['rw'][g] = rw[0]
        fields.append(F)
    y = dict(x, idx=idx, str=strn)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = _results(c, y, fields, 'float64')
        dsig = second_pass(d, x['gq'], o['q32'], o['den32'])['dsig']
    return dict(den=d['den'], q=d['q'], out=d['out'], dsig=dsig)
