"""CPU: the tensor arena itself (tests/tensor_arena.py), with cpu=True so that CPU allocations are guarded -- layout,
alignment, dtype / shape round trips, the pass-through rules, gradient flow through put(), verify()'s wording, views
that outlive their records -- and planted-bug "operators" in plain torch, each run like a GPU case (production, flavour
1, flavour 2; bands, finiteness where production is finite, bit equality with production) and flagged by:

  a store one element past the end / before the start      bands, both flavours
  a store of zeros past the end                            bands, both flavours (no band byte is 0x00)
  a store of 0xFF bytes past the end                       bands, flavour 2 only (flavour 1's bands are 0xFF)
  one row left unwritten                                   flavour 1: not finite; flavour 2: differs from production
  one element fetched past the end, added to the result    flavour 1: not finite (flavour 2: no claim, band bytes read
                                                           as a float may be too small to move the sum)
  the same, scaled by 1e-30 before the add                 flavour 1: not finite (NaN survives any scale; flavour 2: no
                                                           claim, scaled noise mostly vanishes in the sum -- the reason
                                                           flavour 1 poisons with NaN and not with noise)
  one int32 count fetched past the end, added              both flavours differ from production (-1 / band bytes)
  a 128-row tile copied whole from a 100-row input         bands, flavour 2 only: the input's rear band lands on the
    into a 100-row output                                  output's, and in flavour 1 the two are equal

A clean operator passes both.  The planted operators run under the arena only; "production" is the clean operator's
result, which is what a cached block with last call's data, or a harmless neighbour, makes such a bug look like."""
import inspect

import pytest
import torch

import workspace_arena
from tensor_arena import ALIGN, BAND, TensorArena

BAND_T = 1 << 16         # CPU tests: 64 KiB bands (a 128 x 64 float32 tile is 32 KiB)
FILE = "test_tensor_arena_host.py"


def _arena(flavour, m, **kw):
    return TensorArena(flavour, kw.pop("band", BAND_T), cpu=True, **kw).install(m)


def _whole(arena, i=-1):
    return arena.records[i][3]


# ---- layout and round trips --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", [1, 2])
def test_layout_alignment_and_poison(monkeypatch, flavour):
    assert BAND == 1 << 20 and BAND % ALIGN == 0
    arena = _arena(flavour, monkeypatch)
    t = torch.empty((7, 3), dtype=torch.float32, device="cpu")
    site, nbytes, serial, buf = arena.records[0]
    assert nbytes == 7 * 3 * 4 and buf.dtype == torch.uint8 and buf.numel() == BAND_T + nbytes + BAND_T
    assert t.is_contiguous() and t.shape == (7, 3) and t._base is None
    assert t.data_ptr() % ALIGN == 0 and t.data_ptr() == buf.data_ptr() + BAND_T
    assert t.data_ptr() + nbytes == buf[BAND_T + nbytes:].data_ptr()          # the last byte abuts the rear band
    if flavour == 1:
        assert bool(t.isnan().all()) and bool((buf == 0xFF).all())
        assert int(torch.empty(3, dtype=torch.int64, device="cpu")[1]) == -1
        assert bool(torch.empty(5, dtype=torch.float16, device="cpu").isnan().all())
        assert bool(torch.empty(5, dtype=torch.float64, device="cpu").isnan().all())
    else:
        assert not bool(t.any())
        front, rear = buf[:BAND_T], buf[BAND_T + nbytes:]
        assert not bool((front == 0).any()) and not bool((front == 0xFF).any()) and not torch.equal(front, rear)
        torch.empty(4, device="cpu")
        other = _whole(arena)
        assert not torch.equal(other[:BAND_T], front) and not torch.equal(other[:BAND_T], rear)
        assert float((front[1:] != front[:-1]).float().mean()) > 0.9           # no flat stretches to hide a store in
    t[:] = 5.0                                    # use of the view inside its bounds, first to last element
    arena.verify()
    assert arena.records == [] and arena.calls >= 1


@pytest.mark.parametrize("flavour", [1, 2])
def test_every_patched_form_round_trips(monkeypatch, flavour):
    arena = _arena(flavour, monkeypatch)
    src = torch.empty((4, 6), dtype=torch.float16, device=torch.device("cpu"))
    made = [
        (src, (4, 6), torch.float16, None),
        (torch.empty(2, 3, 5, device="cpu"), (2, 3, 5), torch.float32, None),
        (torch.empty([9], dtype=torch.int32, device="cpu"), (9,), torch.int32, None),
        (torch.empty(torch.Size((0, 4)), device="cpu"), (0, 4), torch.float32, None),
        (torch.empty((), dtype=torch.float64, device="cpu"), (), torch.float64, None),
        (torch.zeros(5, dtype=torch.int64, device="cpu"), (5,), torch.int64, 0),
        (torch.zeros((3, 2), device="cpu"), (3, 2), torch.float32, 0),
        (torch.ones(3, dtype=torch.bool, device="cpu"), (3,), torch.bool, True),
        (torch.ones((2, 2), device="cpu"), (2, 2), torch.float32, 1),
        (torch.full((4,), 7, device="cpu"), (4,), torch.int64, 7),
        (torch.full((4,), -2.5, device="cpu"), (4,), torch.float32, -2.5),
        (torch.full((2, 2), 3, dtype=torch.uint8, device="cpu"), (2, 2), torch.uint8, 3),
        (torch.empty_like(src), (4, 6), torch.float16, None),
        (torch.empty_like(src, dtype=torch.int32), (4, 6), torch.int32, None),
        (torch.zeros_like(src), (4, 6), torch.float16, 0),
        (src.new_empty((3,)), (3,), torch.float16, None),
        (src.new_empty(2, 2, dtype=torch.float32), (2, 2), torch.float32, None),
        (src.new_zeros((3, 1)), (3, 1), torch.float16, 0),
        (src.new_zeros(8, dtype=torch.int32), (8,), torch.int32, 0),
    ]
    assert arena.calls == len(made) == len(arena.records)
    for i, (t, shape, dtype, value) in enumerate(made):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu", i
        assert t.data_ptr() % ALIGN == 0 or t.numel() == 0, i
        assert arena.records[i][1] == t.numel() * t.element_size(), i
        if value is not None:
            assert bool((t == value).all()), i
        elif t.numel():
            assert bool((t.view(-1).view(torch.uint8) == arena.poison).all()), i
    leaf = torch.zeros(3, device="cpu", requires_grad=True)
    assert leaf.requires_grad and leaf.is_leaf
    leaf.sum().backward()
    assert torch.equal(leaf.grad, torch.ones(3))
    arena.verify()


def test_pass_through_rules(monkeypatch):
    real_empty = torch.empty
    with monkeypatch.context() as m:
        host = TensorArena(1, BAND_T).install(m)                       # cpu=False: what the GPU tests install
        assert torch.empty is not real_empty
        a = torch.empty(4, device="cpu")
        b, c, d = torch.zeros(4), torch.ones((2,), device=torch.device("cpu")), torch.full((2,), 1.5)
        assert host.calls == 0 and not bool(b.any()) and bool((c == 1).all()) and bool((d == 1.5).all())
        assert host.put(a) is a and a.new_empty(3).shape == (3,) and torch.empty_like(a).shape == (4,)
        assert host.calls == 0 and host.records == []
        host.verify()
    with monkeypatch.context() as m:
        arena = _arena(1, m)
        out = real_empty(6)
        assert torch.empty(6, out=out) is out and arena.calls == 0                # out=
        torch.empty(3, device="meta")                                             # neither CPU nor the GPU
        strided = real_empty(4, 6).t()
        assert torch.empty_like(strided).stride() == strided.stride() and arena.calls == 0     # layout is preserved
        assert torch.empty((2, 3, 4, 5), memory_format=torch.channels_last).stride() == (60, 1, 15, 3)
        assert arena.calls == 0
        ws = workspace_arena.Arena(0x00, guard=256)                               # the workspace arena's own buffers
        view = ws(100, "cpu")
        assert arena.calls == 0 and view.numel() == 100
        ws.verify()
        assert torch.empty(2, device="cpu").shape == (2,) and arena.calls == 1
        arena.verify()
    assert torch.empty is real_empty and torch.Tensor.new_zeros(a, 2).shape == (2,)     # undone with the context


def test_put_copies_and_lets_the_gradient_through(monkeypatch):
    arena = _arena(1, monkeypatch)
    x = torch.arange(12, dtype=torch.float32).view(3, 4).t()         # not contiguous: the copy is
    p = arena.put(x)
    buf = _whole(arena)
    assert torch.equal(p, x) and p.is_contiguous() and p.data_ptr() % ALIGN == 0 and not p.requires_grad
    assert p.data_ptr() + 48 == buf[BAND_T + 48:].data_ptr()
    idx = arena.put(torch.tensor([3, 1, 2], dtype=torch.int32))
    assert idx.dtype == torch.int32 and idx.tolist() == [3, 1, 2]
    leaf = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    placed = arena.put(leaf)
    assert placed.requires_grad and placed.data_ptr() != leaf.data_ptr()
    (placed * torch.tensor([2.0, 3.0, 4.0])).sum().backward()
    assert torch.equal(leaf.grad, torch.tensor([2.0, 3.0, 4.0]))
    arena.verify()


def _ask(n):
    return torch.empty(n, dtype=torch.uint8, device="cpu"), inspect.currentframe().f_lineno


@pytest.mark.parametrize("flavour", [1, 2])
@pytest.mark.parametrize("side", ["before", "after"])
def test_verify_names_site_bytes_side_and_offset(monkeypatch, side, flavour):
    arena = _arena(flavour, monkeypatch)
    _ask(64)
    t, line = _ask(512)
    buf = _whole(arena)
    where = BAND_T - 1 if side == "before" else 0
    at = where if side == "before" else BAND_T + 512
    buf[at] = buf[at] ^ 0x5A
    assert arena.damage() == [(f"{FILE}:_ask:{line}", 512, side, where)]
    with pytest.raises(AssertionError) as e:
        arena.verify()
    msg = str(e.value)
    assert f"{FILE}:_ask:{line}" in msg and "512 bytes" in msg and side in msg and f"offset {where}" in msg
    assert arena.records == [] and (FILE, line) in arena.sites            # released either way
    t[:] = 1                                                              # the view outlives its record
    assert int(t.sum()) == 512


def test_verify_every_bounds_the_records(monkeypatch):
    arena = _arena(2, monkeypatch, verify_every=4)
    kept = [torch.empty(16, device="cpu") for _ in range(11)]
    assert len(arena.records) == 3 and arena.calls == 11
    for i, t in enumerate(kept):                   # released records keep live views valid
        t.fill_(float(i))
    assert [float(t[15]) for t in kept] == [float(i) for i in range(11)]
    _past(torch.empty(16, device="cpu")).fill_(1.0)           # damage, found by the automatic verify
    with pytest.raises(AssertionError, match="after"):
        torch.empty(1, device="cpu")


def test_install_empties_the_module_caches_and_restores_them(monkeypatch):
    from superpoints_registration_amd import ops
    marks = {n: getattr(ops, n) for n in ("_zero_pool", "_NORM_BOUNDS", "_seg_perm_cache")}
    ops._NORM_BOUNDS["sentinel"] = 1
    try:
        with monkeypatch.context() as m:
            _arena(1, m)
            for n, old in marks.items():
                assert getattr(ops, n) == {} and getattr(ops, n) is not old, n
        for n, old in marks.items():
            assert getattr(ops, n) is old, n
        assert ops._NORM_BOUNDS["sentinel"] == 1
    finally:
        del ops._NORM_BOUNDS["sentinel"]


# ---- planted bugs ------------------------------------------------------------------------------------------------------
ROWS, COLS, TILE = 100, 64, 128


def _past(t, k=1, back=False):
    """k elements just behind (or in front of) a tensor's storage range, as an operator indexing out of range sees it."""
    off = t.storage_offset() - k if back else t.storage_offset() + t.numel()
    return t.as_strided((k,), (1,), off)


def op_clean(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


def op_store_past_end(x):
    out = op_clean(x)
    _past(out).fill_(1.0)
    return out


def op_store_before_start(x):
    out = op_clean(x)
    _past(out, back=True).fill_(1.0)
    return out


def op_store_zeros_past_end(x):
    out = op_clean(x)
    _past(out, 4).fill_(0.0)
    return out


def op_store_ff_past_end(x):
    out = op_clean(x)
    _past(out, 4).view(torch.uint8).fill_(0xFF)
    return out


def op_row_unwritten(x):
    out = torch.empty((ROWS, COLS), dtype=torch.float32, device="cpu")
    out[:ROWS - 1] = x[:ROWS - 1] * 2
    return out


def op_fetch_past_end(x):
    out = op_clean(x)
    out[-1, -1] += _past(x)[0]
    return out


def op_fetch_past_end_scaled(x):
    out = op_clean(x)
    out[-1, -1] += _past(x)[0] * 1e-30
    return out


def op_fetch_count_past_end(x):
    out = op_clean(x)
    counts = torch.zeros(8, dtype=torch.int32, device="cpu")
    out[0, 0] += float(_past(counts)[0])
    return out


def op_tile_copy(x):
    out = torch.empty_like(x)
    out.as_strided((TILE, COLS), (COLS, 1), out.storage_offset()).copy_(
        x.as_strided((TILE, COLS), (COLS, 1), x.storage_offset()))
    return out.mul_(2)


def _flagged(monkeypatch, op):
    """Runs op like a GPU case; {flavour: what tripped first} in the order of checking: 'bands', 'finite', 'bits'."""
    g = torch.Generator().manual_seed(3)
    host = torch.rand(ROWS, COLS, generator=g) + 0.5
    production = op_clean(host)
    out = {}
    for flavour in (1, 2):
        with monkeypatch.context() as m:
            arena = _arena(flavour, m)
            got = op(arena.put(host))
        out[flavour] = None
        try:
            arena.verify()
        except AssertionError as e:
            assert f"{FILE}:op_" in str(e)
            out[flavour] = "bands"
            continue
        if not bool(torch.isfinite(got).all()):
            out[flavour] = "finite"
        elif not torch.equal(got.view(-1).view(torch.uint8), production.view(-1).view(torch.uint8)):
            out[flavour] = "bits"
    return out


ANY = "no claim"


@pytest.mark.parametrize("op,expect", [
    (op_clean, {1: None, 2: None}),
    (op_store_past_end, {1: "bands", 2: "bands"}),
    (op_store_before_start, {1: "bands", 2: "bands"}),
    (op_store_zeros_past_end, {1: "bands", 2: "bands"}),
    (op_store_ff_past_end, {1: None, 2: "bands"}),
    (op_row_unwritten, {1: "finite", 2: "bits"}),
    (op_fetch_past_end, {1: "finite", 2: ANY}),
    (op_fetch_past_end_scaled, {1: "finite", 2: ANY}),
    (op_fetch_count_past_end, {1: "bits", 2: "bits"}),
    (op_tile_copy, {1: None, 2: "bands"}),
], ids=lambda v: v.__name__ if callable(v) else "")
def test_planted_bugs_are_flagged_by_the_flavours_named(monkeypatch, op, expect):
    got = _flagged(monkeypatch, op)
    for flavour, want in expect.items():
        assert want is ANY or got[flavour] == want, (flavour, got)
