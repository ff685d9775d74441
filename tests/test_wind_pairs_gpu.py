"""k_wind's paired column walk (two cells per lane, two pressure levels per 16-byte load; sb_set_wind_pairs) against the
one-cell walk it replaces: the same inputs with the knob on and off leave all four outputs bit-identical, after a first
call (the strip kernel compacts k_wind's segment lists) and after a second (the first call's lists stand, unless the plan
cache is off), and last_wind_pairs() tells which instance ran.  The level is also held to a plain numpy first strict minimum on columns without NaN or infinity; columns
with NaN are held to the one-cell walk alone (minloc over NaN is the compiler's choice, no yardstick).

u = 0 and v[k] = -(k+1)/4, so the wind speed a call leaves at a band cell is (level+1)/4 exactly; the state starts at
zero, so the cells a call updated are those with a wind speed.  The mask is built directly: |mask| = 10 in the band, 500
outside it, positive south of a straight coast along the middle row and negative north of it, so that every window
finds both classes within 12 rows.  Grids are at most 192 x 24 cells.
"""
import numpy as np
import pytest
import torch

import wind_trigger_ref as wr
from seabreeze_param_amd import hip

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TS_S = 1800.0
NY = 24
NZS = (1, 2, 3, 13, 14, 15, 29, 56, 57)
# instruction i of the paired walk holds levels 2i and 2i+1; a batch is SB_WIND_UN_PAIR instructions (4, 7 and 14 were
# built and measured): levels 7|8, 13|14 and 27|28 lie on the two sides of a batch boundary of one of them
TIES = ((4, 5), (5, 6), (7, 8), (13, 14), (27, 28))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context()
    yield c
    c.close()


def band_pattern(nx, ny=NY):
    """The band cells (ny, nx): runs that start at an even and at an odd column, inside one 64-cell segment and across
    two; lengths 1, 2, 27, 28, 63, 64; two runs one cell apart; single cells whose pair partner is outside the band;
    the four edges and the last cell of the grid; one whole row."""
    b = np.zeros((ny, nx), bool)
    b[0, 0:3] = True
    b[0, nx - 3:nx] = True
    b[ny - 1, 0] = True
    b[ny - 1, nx - 1] = True                       # its top-level pair is the last 16 bytes of p
    row = 1
    for start in (70, 71):                         # 70 + 64 = 134: the long runs end in the next segment
        for n in (1, 2, 27, 28, 63, 64):
            b[row, start:start + n] = True
            row += 1
    b[row, 10:15] = True; b[row, 16:21] = True     # one cell apart, even start
    b[row, 33:36] = True; b[row, 37:41] = True     # one cell apart, odd start
    b[row, 130:158] = True                         # 28 cells inside the third segment
    row += 1
    for x in (5, 8, 63, 64, 100, 103, 127, 128):   # single cells on both sides of the segment borders
        b[row, x] = True
    row += 1
    b[row, :] = True
    assert row < ny - 1
    return b


def mask_of(band, halo, dt):
    ny, nx = band.shape
    m = np.full((ny + 2 * halo, nx + 2 * halo), 500.0, dt)
    m[halo:halo + ny, halo:halo + nx][band] = 10.0
    m[(ny + 2 * halo) // 2:] *= -1.0
    return m


def columns(nz):
    """[(name, p column)] around the target 70000 Pa; differences are multiples of 250 Pa, exact in single precision."""
    k, last = np.arange(nz), nz - 1
    alt = np.where(k % 2 == 0, 1.0, -1.0)

    def col(d, sign=alt):
        return wr.TARGET_PLEV + 250.0 * np.asarray(d, F64) * sign

    out = []
    for at in (0, 1, nz - 2, last):
        at = min(max(at, 0), last)
        out.append((f"min_at_{at}", col(np.abs(k - at) + 1)))
    for a, b in TIES:
        a, b = min(a, last), min(b, last)
        d = np.minimum(np.abs(k - a), np.abs(k - b)) + 1
        out.append((f"tie_{a}_{b}", col(d, np.ones(nz))))                              # the same value twice
        out.append((f"midway_{a}_{b}", col(2 * d - 1, np.where(k <= a, 1.0, -1.0))))    # the target midway between two levels
    out.append(("constant", col(np.full(nz, 3))))
    out.append(("non_monotone", col((k * 7) % 11 + 1)))
    lo, hi = min(2, last), min(9, last)
    out.append(("two_minima", col(np.minimum(np.abs(k - lo) + 2, np.abs(k - hi) + 1))))
    base = col(np.abs(k - min(3, last)) + 1)
    for name, at in (("nan_at_0", 0), ("nan_at_1", min(1, last)), ("nan_mid", nz // 2), ("nan_at_min", min(3, last))):
        c = base.copy(); c[at] = np.nan
        out.append((name, c))
    out.append(("all_nan", np.full(nz, np.nan)))
    out.append(("all_inf", np.full(nz, np.inf)))
    c = base.copy(); c[min(2, last)] = -np.inf
    out.append(("minus_inf", c))
    c = base.copy(); c[0] = np.inf
    out.append(("inf_at_0", c))
    return out


def level_grid(cols, nx, ny, dt):
    """wr.level_grid for columns that may hold NaN: the columns cycled along longitude, shifted by one per row."""
    nz = cols[0][1].size
    pat = (np.arange(nx)[None, :] + np.arange(ny)[:, None]) % len(cols)
    stack = np.stack([c[1] for c in cols], axis=1)
    p = np.ascontiguousarray(stack[:, pat], dtype=dt)
    assert np.array_equal(p.astype(F64), stack[:, pat], equal_nan=True)                 # exact in dt
    u = np.zeros((nz, ny, nx), dt)
    v = np.ascontiguousarray(np.broadcast_to((-(np.arange(nz) + 1) / 4.0)[:, None, None], (nz, ny, nx)), dtype=dt)
    return p, u, v, pat


def fields(nx, nz, dt, ny=NY):
    """p, u, v and the numpy level (-1 where the column holds a NaN or an infinity)."""
    cols = columns(nz)
    p, u, v, pat = level_grid(cols, nx, ny, dt)
    finite = np.isfinite(p).all(axis=0)
    with np.errstate(invalid="ignore"):
        lev = np.argmin(np.abs(p.astype(F64) - wr.TARGET_PLEV), axis=0)                 # the first of equal minima
    return p, u, v, np.where(finite, lev, -1), [c[0] for c in cols], pat


def flat_fields(mask, dt):
    theta = np.where(mask > 0, 289.0, 288.0).astype(dt)
    return theta, np.zeros_like(theta), (np.arange(theta.size).reshape(theta.shape) % 5).astype(dt)


def run(ctx, pairs, p, u, v, mask, halo=0, bnd=hip.SB_BND_GLOBAL, calls=(1, 2)):
    """-> ([the four outputs after each call], [last_wind_pairs() after each call])"""
    dt = p.dtype
    theta, z, sigma = flat_fields(mask, dt)
    state = [np.zeros(p.shape[1:], dt) for _ in range(4)]
    outs, ran = [], []
    ctx.set_wind_pairs(pairs)
    try:
        for tn in calls:
            ctx.seabreeze_diag(TS_S, tn, p, u, v, theta, mask, z, sigma, *state, halo=halo, bnd=bnd)
            ran.append(ctx.last_wind_pairs())
            outs.append([a.copy() for a in state])
    finally:
        ctx.set_wind_pairs(True)
    return outs, ran


def same_bits(on, off, what):
    for c, (a, b) in enumerate(zip(on, off)):
        for nm, x, y in zip(("windspeed", "winddir", "thc", "sb_con"), a, b):
            diff = np.argwhere(x.view(f"u{x.itemsize}") != y.view(f"u{y.itemsize}"))
            print(f"{what}, call {c + 1}, {nm}: {len(diff)} cells differ; first: {[tuple(int(i) for i in d) for d in diff[:4]]}")
            assert len(diff) == 0, (what, c + 1, nm)


def check_levels(outs, band, lev, names, pat, what):
    for c, o in enumerate(outs):
        ws = o[0]
        assert np.array_equal(ws != 0, band), f"{what}, call {c + 1}: the cells with a wind speed are not the band"
        sel = band & (lev >= 0)
        got = ws[sel].astype(F64) * 4 - 1
        wrong = sorted({names[i] for i in pat[sel][got != lev[sel]]})
        print(f"{what}, call {c + 1}: {int(sel.sum())} finite band columns, patterns with a wrong level: {wrong}")
        assert not wrong, (what, c + 1, wrong)


def both(ctx, p, u, v, band, lev, names, pat, what, eligible, halo=0, bnd=hip.SB_BND_GLOBAL):
    mask = mask_of(band, halo, p.dtype)
    on, ran_on = run(ctx, True, p, u, v, mask, halo, bnd)
    off, ran_off = run(ctx, False, p, u, v, mask, halo, bnd)
    print(f"{what}: last_wind_pairs with the knob on {ran_on}, off {ran_off}")
    assert ran_on == [1 if eligible else 0] * 2 and ran_off == [0, 0], (what, ran_on, ran_off)
    same_bits(on, off, what)
    check_levels(on, band, lev, names, pat, what + ", knob on")
    check_levels(off, band, lev, names, pat, what + ", knob off")
    return on


@pytest.mark.parametrize("nz", NZS)
def test_pairs_match_the_one_cell_walk(ctx, nz):
    """Every band pattern x every column, per level count: odd counts, fewer levels than a batch, a batch and one more,
    the workload's 56."""
    nx = 192
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F64)
    for name in names:                               # every column meets band cells of both parities, and a lone one
        cells = band & (pat == names.index(name))
        assert cells[:, 0::2].any() and cells[:, 1::2].any(), name
    both(ctx, p, u, v, band, lev, names, pat, f"nz={nz}", True)


@pytest.mark.parametrize("mode", ["no_plan_cache", "two_workgroups"])
def test_both_list_paths(ctx, mode):
    """The strip kernel plans every call (k_wind never takes the lists that stand) / two workgroups per kernel (eight
    workgroups of k_wind: every wave walks many segments)."""
    nx, nz = 192, 56
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F64)
    try:
        if mode == "no_plan_cache":
            ctx.set_plan_cache(False)
        else:
            ctx.set_workgroups(2)
        both(ctx, p, u, v, band, lev, names, pat, mode, True)
    finally:
        ctx.set_plan_cache(True)
        ctx.set_workgroups(0)


def test_odd_nx_is_not_eligible(ctx):
    nx, nz = 191, 15
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F64)
    both(ctx, p, u, v, band, lev, names, pat, "nx=191", False)


@pytest.mark.parametrize("h,eligible", [(1, False), (2, True)])
def test_ghost_width(ctx, h, eligible):
    """SB_BND_HALO: an odd ghost width puts the pairs of the frame's segments across interior pairs."""
    nx, nz = 192, 15
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F64)
    both(ctx, p, u, v, band, lev, names, pat, f"halo {h}", eligible, halo=h, bnd=hip.SB_BND_HALO)


def test_single_precision_is_not_eligible(ctx):
    nx, nz = 192, 29
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F32)
    both(ctx, p, u, v, band, lev, names, pat, "float32", False)


def test_p_off_a_16_byte_boundary_is_not_eligible(ctx):
    """Device pointers: p at data_ptr() of its buffer (eligible) and 8 bytes further in a buffer one element longer."""
    nx, nz = 192, 57
    band = band_pattern(nx)
    p, u, v, lev, names, pat = fields(nx, nz, F64)
    mask = mask_of(band, 0, F64)
    theta, z, sigma = flat_fields(mask, F64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: up(a) for k, a in dict(u=u, v=v, theta=theta, mask=mask, z=z, sigma=sigma).items()}
    longer = torch.zeros(p.size + 1, dtype=torch.float64, device="cuda")
    longer[1:].copy_(torch.from_numpy(p.reshape(-1)))
    aligned = up(p)
    assert aligned.data_ptr() % 16 == 0 and longer.data_ptr() % 16 == 0
    res = {}
    for what, p_ptr, eligible in (("aligned", aligned.data_ptr(), 1), ("off by 8 bytes", longer.data_ptr() + 8, 0)):
        for pairs in (True, False):
            state = [torch.zeros((NY, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            ctx.set_wind_pairs(pairs)
            try:
                ctx.seabreeze_diag_dev(F64, TS_S, 1, nx, NY, nz, 0, hip.SB_BND_GLOBAL, p_ptr, d["u"].data_ptr(), d["v"].data_ptr(),
                                       d["theta"].data_ptr(), d["mask"].data_ptr(), d["z"].data_ptr(), d["sigma"].data_ptr(),
                                       *[s.data_ptr() for s in state], stream=hip.torch_stream_handle(torch))
                ran = ctx.last_wind_pairs()
            finally:
                ctx.set_wind_pairs(True)
            torch.cuda.synchronize()
            print(f"p {what}, knob {'on' if pairs else 'off'}: last_wind_pairs {ran}")
            assert ran == (eligible if pairs else 0), (what, pairs, ran)
            res[what, pairs] = [[s.cpu().numpy() for s in state]]
        same_bits(res[what, True], res[what, False], f"p {what}")
        check_levels(res[what, True], band, lev, names, pat, f"p {what}")
    same_bits(res["aligned", True], res["off by 8 bytes", True], "aligned against off by 8 bytes")


def test_um_level_walk_is_not_eligible(ctx):
    """level_rule = 1 (the UM copy's upward walk) through the UM entry point, ghost width 2; the same call with the
    first-minimum rule is eligible."""
    nx, ny, nz, hs, hl, dt = 192, NY, 15, 2, 5, F64
    band = band_pattern(nx, ny)
    mask_l = mask_of(band, hl, dt)
    mask_s = np.ascontiguousarray(mask_l[hl - hs:hl + ny + hs, hl - hs:hl + nx + hs])
    theta_s, z_s, sg_s = flat_fields(mask_s, dt)
    ucols = wr.um_columns(nz)
    for flags, cols, eligible in ((hip.SB_UM_LEVEL_WALK, ucols, 0), (0, columns(nz), 1)):
        p, u, v, pat = level_grid(cols, nx, ny, dt)
        res = {}
        for pairs in (True, False):
            state = [np.zeros((ny, nx), dt) for _ in range(4)]
            ctx.set_wind_pairs(pairs)
            try:
                err = ctx.seabreeze_diag_um(TS_S, 1, p, u, v, theta_s.copy(), z_s, sg_s, mask_l, *state, halo_s=hs, halo_l=hl, flags=flags)
                ran = ctx.last_wind_pairs()
            finally:
                ctx.set_wind_pairs(True)
            print(f"UM entry point, flags {flags}, knob {'on' if pairs else 'off'}: last_wind_pairs {ran}")
            assert err == 0 and ran == (eligible if pairs else 0), (flags, pairs, ran)
            res[pairs] = [state]
        same_bits(res[True], res[False], f"UM entry point, flags {flags}")
        ws = res[True][0][0]
        assert np.array_equal(ws != 0, band)
        if flags:
            lev, defined = wr.um_walk_level(p, wr.TARGET_PLEV, dt)
            sel = band & defined
            assert np.array_equal(ws[sel] * 4 - 1, lev[sel].astype(dt))
        else:
            finite = np.isfinite(p).all(axis=0)
            with np.errstate(invalid="ignore"):
                lev = np.argmin(np.abs(p - wr.TARGET_PLEV), axis=0)
            sel = band & finite
            assert np.array_equal(ws[sel] * 4 - 1, lev[sel].astype(dt))
