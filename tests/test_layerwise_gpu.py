"""The layer-wise GAR kernels (gar_layerwise.hip) called directly on an adversarial segment table
(_layerwise_common.py): segments shorter than a group, unaligned starts, job edges inside 8-wide
groups, base != 0. On the exact inputs the expected result is the fp64 oracle bit for bit; sharded
and arbitrarily cut launches must give the bits of the whole-table launch."""
import pytest
import torch

import _layerwise_common as lw

pytestmark = pytest.mark.gpu

NAN = float("nan")
_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16", None: "none"}
dtypes = pytest.mark.parametrize("dtype", lw.DTYPES, ids=[_NAME[d] for d in lw.DTYPES])


def jobs_on(cut_range, dev):
    return lw.job_tensors(cut_range[2], cut_range[3], dev)


# ---------------------------------------------------------------------------------------------
# A. gpu_lw_gram

def run_gram(native, Xd, cut, n):
    """One launch per owned range on NaN-filled outputs: the [L, n, n] blocks of every range (fp64, CPU)."""
    np_ = native.gram_padded(n)
    outs = []
    for r in cut:
        J, S = jobs_on(r, Xd.device)
        slabs = torch.full((J.shape[0] * native.gram_slab_floats(n),), NAN, device=Xd.device)
        gram = torch.full((lw.L * np_ * np_,), NAN, device=Xd.device)
        native.gpu_lw_gram(Xd[:, r[0]:r[1]], J, S, slabs, gram)
        outs.append(gram.view(lw.L, np_, np_)[:, :n, :n].cpu().double())
    return outs


def assert_gram(got, want, what):
    if not torch.equal(got, want):
        s, i, j = (got != want).nonzero()[0].tolist()
        raise AssertionError(f"{what}: segment {s} (start {lw.OFFS[s]}, length {lw.LENS[s]}) entry ({i}, {j}): "
                             f"got {got[s, i, j].item()!r}, want {want[s, i, j].item()!r}; "
                             f"{int((got != want).sum())} entries differ")


@pytest.mark.parametrize("kind", sorted(lw.CUTS))
@dtypes
@pytest.mark.parametrize("n", lw.NS)
def test_gram_exact(cuda, native, n, dtype, kind):
    X = lw.gram_exact_rows(n)
    cut = lw.CUTS[kind]()
    outs = run_gram(native, X.to(dtype).to(cuda), cut, n)
    want = lw.gram_fp64(X)
    if kind == "shards":
        for r, got in zip(cut, outs):
            part = lw.gram_fp64(X, r[0], r[1])
            empty = [s for s in range(lw.L) if r[3][s] == r[3][s + 1]]
            assert empty and not part[empty].any()                 # no job: an all-zero block
            assert_gram(got, part, f"range [{r[0]}, {r[1]})")
        assert_gram(sum(outs), want, "sum over the owned ranges")
    else:
        assert_gram(outs[0], want, kind)


@dtypes
@pytest.mark.parametrize("n", lw.NS)
def test_gram_randn_within_the_fp32_sum_bound(cuda, native, n, dtype):
    X = lw.gram_randn_rows(n, dtype)
    got = run_gram(native, X.to(cuda), lw.whole_cut(), n)[0]
    err, bound = (got - lw.gram_fp64(X)).abs(), lw.gram_bound(X)
    ratio = err / bound
    print(f"lw_gram randn n={n} {_NAME[dtype]}: largest error / bound {float(ratio.max()):.4f} "
          f"(segment {int(ratio.flatten(1).amax(1).argmax())})")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------
# B. gpu_lw_combine_sgd

def launch_combine(native, Xd, cut, w, param, mom, shadow, hp, nesterov, first):
    seg_off = lw.seg_off_tensor(Xd.device)
    for r in cut:
        o0, o1 = r[0], r[1]
        J, _ = jobs_on(r, Xd.device)
        sh = None if shadow is None else (shadow if (o0, o1) == (0, lw.D) else shadow[o0:o1])
        native.gpu_lw_combine_sgd(Xd[:, o0:o1], J, seg_off, o0, w, param[o0:o1], mom[o0:o1], sh, hp["lr"],
                                  hp["momentum"], hp["dampening"], hp["weight_decay"], nesterov, first)


def combine_inputs(n, dtype, inputs):
    if inputs == "exact":
        return [lw.combine_exact_rows(n, k).to(dtype) for k in range(2)], lw.exact_weights(n), lw.exact_param(), lw.EXACT_HP
    return [lw.combine_randn_rows(n, k, dtype) for k in range(2)], lw.randn_weights(n), lw.randn_param(), lw.RANDN_HP


def two_steps(native, cuda, n, dtype, kind, inputs, nesterov, shadow_dt, momentum=None, mom_fill=0.0):
    """first_step True then False with fresh rows: (param, mom, shadow) on the CPU after every step."""
    rows, w, p0, hp = combine_inputs(n, dtype, inputs)
    hp = hp if momentum is None else dict(hp, momentum=momentum)
    cut = lw.CUTS[kind]()
    param, wd = p0.to(cuda), w.to(cuda)
    mom = torch.full((lw.D,), mom_fill, device=cuda)
    shadow = None if shadow_dt is None else torch.full((lw.D + 9,), lw.SENTINEL, device=cuda, dtype=shadow_dt)
    out = []
    for k in range(2):
        launch_combine(native, rows[k].to(cuda), cut, wd, param, mom, shadow, hp, nesterov, k == 0)
        out.append((param.clone().cpu(), mom.clone().cpu(), None if shadow is None else shadow.clone().cpu()))
    return out


@pytest.mark.parametrize("shadow_dt", [None, torch.bfloat16, torch.float16], ids=["none", "bf16", "fp16"])
@pytest.mark.parametrize("nesterov", [False, True])
@dtypes
@pytest.mark.parametrize("n", lw.NS)
def test_combine_sgd_exact(cuda, native, n, dtype, nesterov, shadow_dt):
    want, _ = lw.combine_exact_oracle(n, nesterov)
    cut = lw.whole_cut()
    got = two_steps(native, cuda, n, dtype, "whole", "exact", nesterov, shadow_dt)
    for k, ((p, m, sh), (p64, m64)) in enumerate(zip(got, want)):
        lw.assert_same(p.double(), p64, f"param after step {k + 1}", cut)
        lw.assert_same(m.double(), m64, f"momentum after step {k + 1}", cut)
        if sh is not None:
            lw.assert_same(sh[:lw.D], p.to(shadow_dt), f"shadow after step {k + 1}", cut, bitwise=True)
            assert bool((sh[lw.D:] == lw.SENTINEL).all())


@dtypes
def test_combine_sgd_without_momentum_leaves_mom(cuda, native, dtype):
    n = 17
    want, _ = lw.combine_exact_oracle(n, False, 0.0)
    for kind in ("whole", "shards"):
        got = two_steps(native, cuda, n, dtype, kind, "exact", False, None, momentum=0.0, mom_fill=lw.SENTINEL)
        for k, ((p, m, _), (p64, _)) in enumerate(zip(got, want)):
            lw.assert_same(p.double(), p64, f"{kind}: param after step {k + 1}", lw.CUTS[kind]())
            assert bool((m == lw.SENTINEL).all())


@pytest.mark.parametrize("inputs", ["exact", "randn"])
@pytest.mark.parametrize("kind", ["shards", "arbitrary"])
@dtypes
@pytest.mark.parametrize("n", lw.NS)
def test_combine_sgd_cuts_give_the_whole_tables_bits(cuda, native, n, dtype, kind, inputs):
    nesterov = n in (17, 128)
    shadow_dt = torch.float16 if dtype == torch.float16 else torch.bfloat16
    whole = two_steps(native, cuda, n, dtype, "whole", inputs, nesterov, shadow_dt)
    got = two_steps(native, cuda, n, dtype, kind, inputs, nesterov, shadow_dt)
    cut = lw.CUTS[kind]()
    for k, (g, w) in enumerate(zip(got, whole)):
        for name, a, b in zip(("param", "momentum", "shadow"), g, w):
            lw.assert_same(a, b, f"{kind} / {inputs}: {name} after step {k + 1}", cut, bitwise=True)


@dtypes
@pytest.mark.parametrize("n", lw.NS)
def test_combine_sgd_segments_have_the_flat_kernels_bits(cuda, native, n, dtype):
    """The file header's invariant: every segment gets the bits of gpu_combine_sgd run on that segment
    alone (aligned copy of its rows, padded row stride, its own weights)."""
    rows, w, p0, hp = combine_inputs(n, dtype, "randn")
    nesterov = n in (7, 40)
    got = two_steps(native, cuda, n, dtype, "whole", "randn", nesterov, None)
    wd = w.to(cuda)
    for s in range(lw.L):
        a, e = lw.OFFS[s], lw.OFFS[s + 1]
        p, m = p0[a:e].to(cuda).clone(), torch.zeros(e - a, device=cuda)
        for k in range(2):
            Xs = torch.zeros((n, (e - a + 7) // 8 * 8), dtype=dtype, device=cuda)
            Xs[:, :e - a] = rows[k][:, a:e].to(cuda)
            native.gpu_combine_sgd(Xs[:, :e - a], wd[s], p, m, None, None, hp["lr"], hp["momentum"], hp["dampening"],
                                   hp["weight_decay"], nesterov, k == 0)
            lw.assert_same(got[k][0][a:e], p.cpu(), f"segment {s}: param after step {k + 1}", base=a, bitwise=True)
            lw.assert_same(got[k][1][a:e], m.cpu(), f"segment {s}: momentum after step {k + 1}", base=a, bitwise=True)


@pytest.mark.parametrize("nesterov", [False, True])
@dtypes
@pytest.mark.parametrize("n", [7, 17])
def test_flat_combine_sgd_dampening_and_grad_out(cuda, native, n, dtype, nesterov):
    """gpu_combine_sgd with dampening and grad_out on the exact inputs at an odd d (scalar tail)."""
    d = 10007
    w = lw.exact_weights(n)[0]
    rows = [lw.combine_exact_rows(n, k)[:, :d + 1].contiguous() for k in range(2)]
    grads = [w.double() @ X[:, :d].double() for X in rows]
    want = lw.sgd_fp64(lw.exact_param()[:d], grads, lw.EXACT_HP, nesterov)
    hp = lw.EXACT_HP
    param, mom, wd = lw.exact_param()[:d].to(cuda), torch.zeros(d, device=cuda), w.to(cuda)
    shadow = torch.full((d + 9,), lw.SENTINEL, device=cuda, dtype=torch.bfloat16)
    for k in range(2):
        gout = torch.full((d,), NAN, device=cuda)
        Xd = rows[k].to(dtype).to(cuda)
        native.gpu_combine_sgd(Xd[:, :d], wd, param, mom, gout, shadow, hp["lr"], hp["momentum"], hp["dampening"],
                               hp["weight_decay"], nesterov, k == 0)
        for name, got, ref64 in (("grad_out", gout, grads[k]), ("param", param, want[k][0]), ("momentum", mom, want[k][1])):
            bad = (got.cpu().double() != ref64).nonzero().flatten().tolist()
            assert not bad, f"{name} after step {k + 1}: {len(bad)} of {d} differ, first at {bad[:6]}"
        assert torch.equal(shadow[:d].cpu(), param.cpu().to(torch.bfloat16)) and bool((shadow[d:] == lw.SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# C. gpu_lw_bulyan_tail

def run_tail(native, Xd, cut, Wd, t, beta, out, only=None):
    """Launches on ``out`` ([D + 9] fp32); ``only(i, jobs)``: the jobs of range i that run."""
    for i, r in enumerate(cut):
        jobs = r[2] if only is None else only(i, r[2])
        if jobs:
            J, _ = lw.job_tensors(jobs, r[3], Xd.device)
            native.gpu_lw_bulyan_tail(Xd[:, r[0]:r[1]], J, Wd, t, beta, out if (r[0], r[1]) == (0, lw.D) else out[r[0]:r[1]])


TAIL_CASES = ([(s, dt) for s in lw.TAIL_MFMA for dt in (torch.bfloat16, torch.float16)]
              + [(s, torch.float32) for s in lw.TAIL_MFMA] + [(s, torch.bfloat16) for s in lw.TAIL_SCALAR_BF16])


@pytest.mark.parametrize("poisoned", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("shape,dtype", TAIL_CASES, ids=["n%d-t%d-b%d-%s" % (s + (_NAME[dt],)) for s, dt in TAIL_CASES])
def test_bulyan_tail_exact(cuda, native, shape, dtype, poisoned):
    """Every coordinate of every job is reference._closest_mean of its segment's selection means, bit
    for bit; with inf / -inf / NaN in a row that no set contains, still that (the oracle never sees
    the row); coordinates outside the launched jobs keep their sentinel."""
    n, t, beta = shape
    assert lw.tail_mfma_ok(n, t, beta, dtype) == (shape in lw.TAIL_MFMA and dtype != torch.float32)
    want = lw.tail_exact_oracle(n, t, beta)
    X = lw.tail_exact_rows(n)
    Xd = (lw.poison(X) if poisoned else X).to(dtype).to(cuda)
    Wd = lw.tail_exact_W(n, t).to(cuda)
    sent = torch.full((lw.D + 9,), lw.SENTINEL, device=cuda)
    keep = torch.tensor([s % 2 == 0 for s in range(lw.L)]).repeat_interleave(torch.tensor(lw.LENS))   # even segments

    whole = lw.whole_cut()
    out = sent.clone()
    run_tail(native, Xd, whole, Wd, t, beta, out, only=lambda i, jobs: [j for j in jobs if j[2] % 2 == 1])
    got = out.cpu()
    assert bool((got[:lw.D][keep] == lw.SENTINEL).all()) and bool((got[lw.D:] == lw.SENTINEL).all())
    lw.assert_same(got[:lw.D][~keep].double(), want[~keep], "odd segments' jobs alone")
    run_tail(native, Xd, whole, Wd, t, beta, out, only=lambda i, jobs: [j for j in jobs if j[2] % 2 == 0])
    got = out.cpu()
    lw.assert_same(got[:lw.D].double(), want, "whole table", whole)
    assert bool((got[lw.D:] == lw.SENTINEL).all())

    shards = lw.shard_cuts()
    out = sent.clone()
    run_tail(native, Xd, shards, Wd, t, beta, out, only=lambda i, jobs: jobs if i != 2 else [])
    got = out.cpu()
    o0, o1 = shards[2][:2]
    assert bool((got[o0:o1] == lw.SENTINEL).all())
    lw.assert_same(got[:o0].double(), want[:o0], "shard cuts, ranges 0-1", shards)
    lw.assert_same(got[o1:lw.D].double(), want[o1:], "shard cuts, ranges 3-5", shards, base=o1)
    run_tail(native, Xd, shards, Wd, t, beta, out, only=lambda i, jobs: jobs if i == 2 else [])
    got = out.cpu()
    lw.assert_same(got[:lw.D].double(), want, "shard cuts", shards)
    assert bool((got[lw.D:] == lw.SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bulyan_tail_one_long_job_overflows_the_bad_group_list(cuda, native, dtype):
    """One job of 163 840 coordinates with a non-finite value in every 64-group: every wave lists more
    groups than it has slots and redoes all of its groups exactly."""
    n, t, beta = lw.TAIL_MFMA[0]
    d = lw.TAIL_LONG_JOB
    X = lw.tail_exact_rows(n, d)
    W = lw.tail_exact_W(n, t, 1)
    want, _ = lw.closest_mean(lw.tail_means(X, W, 0, 0, d), beta)
    out = torch.full((d + 9,), lw.SENTINEL, device=cuda)
    J = torch.tensor([[0, d, 0]], dtype=torch.int64, device=cuda)
    native.gpu_lw_bulyan_tail(lw.poison_every_group(X).to(dtype).to(cuda), J, W.to(cuda), t, beta, out)
    got = out.cpu()
    bad = (got[:d].double() != want).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} of {d} differ, first at {bad[:8]} (groups {[x // 64 for x in bad[:8]]})"
    assert bool((got[d:] == lw.SENTINEL).all())


def test_bulyan_tail_randn_bulyan_sized_sets(cuda, native):
    X, W, t, beta, want, bound, keep = lw.tail_randn_case()
    out = torch.full((lw.D,), lw.SENTINEL, device=cuda)
    run_tail(native, X.to(cuda), lw.whole_cut(), W.to(cuda), t, beta, out)
    err = (out.cpu().double() - want).abs()
    ratio = (err / bound)[keep]
    print(f"lw_bulyan_tail randn bf16 n={X.shape[0]} t={t} beta={beta}: largest error / bound {float(ratio.max()):.4f}, "
          f"{100 * (1 - float(keep.double().mean())):.4f} % of the coordinates left out (near-tie of the window)")
    assert 1 - float(keep.double().mean()) <= 0.005
    worst = int(torch.where(keep, err / bound, torch.zeros_like(err)).argmax())
    assert bool((err[keep] <= bound[keep]).all()), lw.describe(worst, lw.whole_cut())
