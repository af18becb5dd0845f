"""The tm_gemm sweep's case table, reference and dispatch restatement (tests/gemm_cases.py), checked
without a GPU: the table reaches every kernel variant the product dispatch can launch on a 256-CU
device, every case names the path it takes, and the fp64 reference agrees with independent routes
(the oracle's torch.cat / rearrange forms, the strided reading of the header's A(m,k) / B(k,n))."""
import itertools

import pytest
import torch

import gemm_cases as G
from gemm_cases import BF16, F32, CASES

CU = 256
BY_NAME = {c.name: c for c in CASES}


def _built(case):
    return G.build(case, torch.Generator().manual_seed(5), CU)


@pytest.fixture(scope="module")
def built():
    return {c.name: _built(c) for c in CASES}


def test_every_case_names_the_path_it_takes(built):
    for c in CASES:
        a = built[c.name].args
        assert G.expected_path(a, CU) == (c.path, c.kind), c.name
        if c.m_cu:     # 128-row tiles spill past one per CU, 160-row tiles do not
            t128, t160 = G.tile_counts(a)
            assert t128 > CU >= t160, (c.name, t128, t160)
            assert a["M"] % 160 not in (0, 128)


def test_the_160_row_ring_never_gets_k_zero(built):
    """its first stage is issued before the k-tile count is looked at: the dispatch must keep K = 0 off it"""
    for c in CASES:
        a = dict(built[c.name].args, K=0)
        assert G.expected_path(a, CU)[0] != "ring160", c.name
    c = BY_NAME["ring160-shape-K0-bias-only"]
    a = built[c.name].args
    assert G.expected_path(dict(a, K=64), CU) == ("ring160", "plain") and G.expected_path(a, CU) == ("ring", "plain")


def test_rows_from_the_cu_count_at_256():
    assert G.rows_of(BY_NAME["ring160-plain-nn-K64-bf16"], CU) == 16421      # 258 vs 206 tiles
    assert G.rows_of(BY_NAME["ring160-qkv-dh64"], CU) == 10917               # 3 bags of 3639


def test_table_reaches_every_instantiation_of_the_product_dispatch(built):
    have = {G.instantiation(built[c.name].args, CU) for c in CASES}
    want = set()
    for ab, (at, bkn) in itertools.product((F32, BF16), G.LAYOUTS):
        want.add(("reg", ab, at, bkn))
    for (at, bkn), kind in itertools.product(G.LAYOUTS, ("plain", "any", "qkv", "splitk")):
        want.add(("ring", at, bkn, kind))
    for bkn, out in itertools.product((0, 1), (BF16, F32)):
        want.add(("ring160", bkn, "plain", out))
    want.add(("ring160", 0, "qkv", BF16))
    for out in (BF16, F32):
        want.add(("big", 256, out))
    assert not want - have, sorted(want - have, key=str)
    # and nothing the product cannot launch: the 160-row ring never runs the runtime-mode epilogue
    # or a split, the big tile only the QKV scatter on k-contiguous operands
    assert not [i for i in have if i[0] == "ring160" and i[2] in ("any", "splitk")]
    assert not [i for i in have if i[0] == "big" and i[1] != 256]


def test_features_the_issue_lists_are_in_the_table():
    on = lambda path, f: [c for c in CASES if c.path == path and f(c)]   # noqa: E731
    assert on("ring", lambda c: c.a_off and c.lda_pad)                       # lda > K, offset A
    assert on("ring", lambda c: c.pre == "bf16" and c.out == F32)
    assert on("ring", lambda c: c.seed_dev >= 0 and c.drop_p > 0 and c.resid and c.rowmap[1] > 0)
    assert on("ring", lambda c: c.kind == "qkv" and c.bias)
    assert on("ring", lambda c: c.kind == "any" and c.out == BF16)
    assert on("ring", lambda c: c.accumulate and c.b_kn and not c.resid)
    assert on("ring", lambda c: c.accumulate and c.resid)
    assert on("ring", lambda c: c.kind == "plain" and (c.N % 8 or (c.N + c.ldc_pad) % 8))
    assert on("ring", lambda c: c.kind == "splitk" and c.K % c.kps and c.slab_bf16)
    assert on("ring", lambda c: c.kind == "splitk" and c.splits * c.kps > c.K + c.kps)   # an empty last split
    assert on("reg", lambda c: c.kind == "splitk" and c.K % c.kps == 8)
    assert on("reg", lambda c: c.K % (8 if c.ab == BF16 else 4))             # the per-element k tail
    assert on("reg", lambda c: c.K == 0) and on("ring", lambda c: c.K == 0 and not c.m_cu)
    assert on("ring", lambda c: c.K == 0 and c.m_cu)                         # K = 0 at the 160-row ring's shape
    assert on("ring160", lambda c: c.N % 128 and c.b_kn and c.out == F32)
    assert on("big", lambda c: c.N % 256 and rows_ragged(c))


def rows_ragged(c):
    return c.M % 256 != 0 and (c.M // c.bags) % 256 != 0


def _same(a, b):
    return torch.allclose(a, b, rtol=0, atol=1e-12)


def _strided(buf, off, rows, cols, ld, trans):
    """X(r, c) = trans ? buf[c * ld + r] : buf[r * ld + c], as the header defines A(m,k) and B(k,n)"""
    return torch.as_strided(buf, (rows, cols), (1, ld) if trans else (ld, 1), off).double()


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.m_cu and c.path != "big"])
def test_reference_product_equals_the_headers_strided_reading(name, built):
    """alpha A(m,k) B(k,n) + bias read from the stored buffers by the header's index formulas (pad
    elements are NaN and must not be touched) equals what the reference stores, on every case without
    GELU / dropout / addends; the split-K slabs sum to the full product."""
    c, b = BY_NAME[name], built[name]
    a = b.args
    A = _strided(b.A, c.a_off, a["M"], a["K"], a["lda"], a["a_trans"])
    B = _strided(b.B, 0, a["K"], a["N"], a["ldb"], not a["b_kn"])
    full = A @ B
    assert torch.isfinite(full).all()
    ref = G.reference(c, b)
    if c.kind == "splitk":
        r, m, _ = ref["C"]
        slabs = r[m].view(c.splits, a["M"], a["N"])
        assert torch.allclose(slabs.sum(0), full, rtol=0, atol=1e-12)
        kps = a["k_per_split"]
        for z in range(c.splits):
            assert _same(slabs[z], A[:, z * kps:(z + 1) * kps] @ B[z * kps:(z + 1) * kps])
        if c.colsum:
            r, m, _ = ref["colsum"]
            assert torch.allclose(r[m].view(c.splits, a["M"]).sum(0), A.sum(1), rtol=0, atol=1e-12)
        return
    x = c.alpha * full + (b.bias.double() if c.bias else 0.0)
    if c.pre:
        r, m, _ = ref["pre"]
        assert _same(r[m].view(a["M"], a["N"]), x)
    if c.kind == "plain":
        r, m, _ = ref["C"]
        assert _same(r[m].view(a["M"], a["N"]), x)
        assert int(m.sum()) == a["M"] * a["N"] and m.numel() == (a["M"] + 2) * a["ldc"]


def test_row_map_reference_is_the_oracles_cat_behind_a_class_row(built):
    """h = gelu(x W^T + b) per bag; the model forms cat([cls, h, h[:, :add]], 1) (oracle/transmil_ref.py)."""
    for name in ("ring-any-nn-K64-gelu-pre-dup-f32", "ring-any-nk-K192-gelu-pre_bf16-dup-f32"):
        c, b = BY_NAME[name], built[name]
        Bg, (Nn, _, S, _, add, _) = c.bags, c.rowmap
        ref, mask, _ = G.reference(c, b)["C"]
        x = b.A_log @ b.B_log + b.bias.double()
        h = torch.nn.functional.gelu(x).view(Bg, Nn, c.N)
        cls = torch.full((Bg, 1, c.N), 7.0, dtype=torch.float64)
        want = torch.cat([cls, torch.cat([h, h[:, :add]], 1)], 1)
        got = ref[:Bg * S * c.N].view(Bg, S, c.N).clone()
        m = mask[:Bg * S * c.N].view(Bg, S, c.N)
        assert not m[:, 0].any() and m[:, 1:].all() and not mask[Bg * S * c.N:].any()
        got[:, 0] = 7.0
        assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_skip_row_map_drops_the_front_pad_rows(built):
    c = BY_NAME["ring-any-nk-K128-dropout-resid-skip-f32"]
    b = built[c.name]
    grp_in, skip, grp_out = c.rowmap[:3]
    pairs = G.row_map(c, b.args["M"])
    assert len(pairs) == 2 and pairs[1][0].numel() == 0
    m, r = pairs[0]
    assert m.numel() == c.bags * (grp_in - skip) and torch.equal(r, torch.arange(c.bags * grp_out))
    assert torch.equal(m.view(c.bags, -1)[:, 0], torch.arange(c.bags) * grp_in + skip)


def test_qkv_reference_is_the_rearranged_chunks_with_q_scaled(built):
    """to_qkv(x).chunk(3, -1), each 'b n (h d) -> b h n d', q scaled (the third-party NystromAttention)."""
    for c in CASES:
        if c.kind != "qkv" or c.m_cu or c.path == "big":
            continue
        b = built[c.name]
        nh, dh, qs = c.qkv
        seq = b.args["M"] // c.bags
        x = (b.A_log @ b.B_log + (b.bias.double() if c.bias else 0.0)).view(c.bags, seq, 3 * nh * dh)
        q, k, v = (t.reshape(c.bags, seq, nh, dh).permute(0, 2, 1, 3) for t in x.chunk(3, -1))
        want = torch.stack([q * qs, k, v])
        ref, mask, _ = G.reference(c, b)["C"]
        assert mask[:want.numel()].all() and not mask[want.numel():].any()
        assert torch.allclose(ref[:want.numel()].view_as(want), want, rtol=0, atol=1e-12), c.name


def test_dropout_reference_keeps_about_one_minus_p(built):
    """Checks the inputs (seed, p, the mask's geometry), from the reference mask alone."""
    for c in CASES:
        if c.drop_p <= 0:
            continue
        b = built[c.name]
        keep = G.dropout_keep(c.seed_dev, c.seed, b.out_rows, c.N, c.drop_p)
        assert abs(keep.mean() - (1 - c.drop_p)) < 0.02, c.name
        # and the reference holds exactly the residual where the mask drops
        ref, mask, _ = G.reference(c, b)["C"]
        ldc = b.args["ldc"]
        r = ref.view(-1, ldc)[:b.out_rows, :c.N]
        res = b.resid.double().view(-1, ldc)[:b.out_rows, :c.N]
        dropped = torch.from_numpy(~keep)
        assert torch.equal(r[dropped], res[dropped]) and not torch.equal(r, res)


def test_bound_is_the_issues_formula():
    ref = torch.tensor([4.0, -0.5, 100.0, 0.0], dtype=torch.float64)
    mask = torch.tensor([True, True, False, True])
    assert torch.equal(G.bound(ref, mask, 0.0), torch.full((4,), 4e-5, dtype=torch.float64))
    assert torch.allclose(G.bound(ref, mask, 2.0 ** -8)[:2], torch.tensor([4e-5 + 4 / 256, 4e-5 + 0.5 / 256],
                                                                          dtype=torch.float64), rtol=1e-15)
