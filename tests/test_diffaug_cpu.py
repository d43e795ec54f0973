"""CPU: the DiffAugment pipe's surface, configuration, sampler and the op's torch forms (no kernel runs here).

* registry entry, kwargs dataclass, buffers, strength mirror, `_augment_arguments` for aug.aug_type=diffaug and its two refusals;
* the sampler: determinism under the CPU seed, ranges, p = 0 and p = 1, gate frequencies, the cutout rectangle against the published
  clamped scatter for every offset;
* `diffaug_reference` and the two mutually recursive Functions in float64 against tests/diffaug_util.py, gradcheck / gradgradcheck."""
import math

import pytest
import torch

import style_big_gan_amd
from style_big_gan_amd import arguments
from style_big_gan_amd.torch_utils.ops import diffaug as D
from style_big_gan_amd.train_parts import augmentations as A
from style_big_gan_amd.train_parts.trainers import BaseTrainer

import diffaug_util as U

POLICIES = ["color", "translation", "cutout", "color_translation", "color_cutout", "translation_cutout", "color_translation_cutout"]


@pytest.fixture
def _cfg(tmp_path):
    """the structured defaults (an empty yaml file) with a dot-list on top"""
    (tmp_path / "empty.yaml").write_text("{}\n")
    return lambda *dotlist: arguments.load_config([f"exp.config_dir={tmp_path}", "exp.config=empty.yaml"] + list(dotlist))


def test_registry_and_surface():
    assert "diffaug" in A.augmentations.classes and A.augmentations["diffaug"] is A.DiffAugmentPipe
    args = A.augmentations.args["diffaug"]()
    assert args.translation_ratio == 0.125 and args.cutout_ratio == 0.5 and args.color == 0 and args.translation == 0 and args.cutout == 0
    assert sorted(A.diffaug_specs) == sorted(POLICIES)
    assert A.diffaug_specs["color_translation_cutout"] == dict(color=1, translation=1, cutout=1)
    pipe = A.augmentations["diffaug"](**A.diffaug_specs["color_translation_cutout"])
    assert [k for k, _ in pipe.named_buffers()] == ["p"] and list(pipe.state_dict().keys()) == ["p"] and not list(pipe.parameters())
    assert pipe._strength() == 1.0
    pipe.p.copy_(torch.as_tensor(0.25))                 # an in-place write nobody announced: the mirror follows
    assert pipe._strength() == 0.25
    pipe.p.copy_(torch.as_tensor(0.5))
    pipe.announce_strength_update()
    pipe.adopt_strength()
    assert pipe._strength() == 0.5
    # the ADA pipe shares the mirror and keeps its buffers
    ada = A.augmentations["sg2_ada"](**A.augpipe_specs["bgc"])
    assert isinstance(ada, A._StrengthPipe) and sorted(k for k, _ in ada.named_buffers()) == ["Hz_fbank", "Hz_geom", "p"]
    ada.p.copy_(torch.as_tensor(0.125))
    assert ada._strength() == 0.125


def test_augment_arguments_select_the_policy_table(_cfg):
    out = BaseTrainer._augment_arguments(_cfg("aug.aug_type=diffaug", "aug.aug=fixed", "aug.p=1", "aug.augpipe=color_translation_cutout"))
    assert out["augment_type"] == "diffaug" and out["augment_p"] == 1.0 and out["ada_target"] is None
    assert out["augment_kwargs"] == dict(color=1, translation=1, cutout=1, translation_ratio=0.125, cutout_ratio=0.5)
    A.augmentations["diffaug"](**out["augment_kwargs"])
    out = BaseTrainer._augment_arguments(_cfg("aug.aug_type=diffaug", "aug.aug=ada", "aug.augpipe=translation"))
    assert out["ada_target"] == 0.6 and out["augment_p"] == 0.0 and out["augment_kwargs"]["translation"] == 1 and out["augment_kwargs"]["color"] == 0
    out = BaseTrainer._augment_arguments(_cfg("aug.aug_type=diffaug", "aug.aug=noaug"))
    assert out["augment_kwargs"] is None
    with pytest.raises(ValueError, match="sg2_ada") as e:           # unknown type: the registered names
        BaseTrainer._augment_arguments(_cfg("aug.aug_type=nothing", "aug.aug=fixed", "aug.p=1"))
    assert "diffaug" in str(e.value)
    with pytest.raises(ValueError, match="color_translation_cutout"):       # the default 'bgc' is no DiffAugment policy
        BaseTrainer._augment_arguments(_cfg("aug.aug_type=diffaug", "aug.aug=fixed", "aug.p=1"))
    with pytest.raises(ValueError, match="bgcfnc"):
        BaseTrainer._augment_arguments(_cfg("aug.aug=fixed", "aug.p=1", "aug.augpipe=color_translation_cutout"))
    # sg2_ada as before
    ada = BaseTrainer._augment_arguments(_cfg())
    assert ada["augment_type"] == "sg2_ada" and ada["ada_target"] == 0.6 and ada["augment_p"] == 0.0
    assert {k for k, v in ada["augment_kwargs"].items() if v == 1 and k in A.augpipe_specs["bgcfnc"]} == set(A.augpipe_specs["bgc"])
    fixed = BaseTrainer._augment_arguments(_cfg("aug.aug=fixed", "aug.p=0.3", "aug.augpipe=bg"))
    assert fixed["augment_p"] == 0.3 and fixed["augment_kwargs"]["xflip"] == 1 and fixed["augment_kwargs"]["hue"] == 0
    assert sorted(A.augpipe_specs) == sorted(["blit", "geom", "color", "filter", "noise", "cutout", "bg", "bgc", "bgcf", "bgcfn", "bgcfnc"])


def test_sampler_ranges_and_determinism():
    pipe = A.DiffAugmentPipe(color=1, translation=1, cutout=1)
    N, C, H, W = 512, 3, 13, 32
    torch.manual_seed(3)
    a = pipe.sample(N, C, H, W)
    torch.manual_seed(3)
    b = pipe.sample(N, C, H, W)
    assert all(torch.equal(a[k], b[k]) for k in a) and sorted(a) == ["b", "k", "rect", "s", "t"]
    assert all(v.device.type == "cpu" for v in a.values())
    assert a["b"].dtype == torch.float32 and a["t"].dtype == torch.int32 and a["rect"].dtype == torch.int32
    assert tuple(a["t"].shape) == (N, 2) and tuple(a["rect"].shape) == (N, 4)
    assert -0.5 <= float(a["b"].min()) and float(a["b"].max()) < 0.5 and float(a["b"].max() - a["b"].min()) > 0.9
    assert 0 <= float(a["s"].min()) and float(a["s"].max()) < 2 and float(a["s"].max()) > 1.8
    assert 0.5 <= float(a["k"].min()) and float(a["k"].max()) < 1.5 and float(a["k"].max()) > 1.4
    lim_h, lim_w = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
    assert (lim_h, lim_w) == (2, 4)
    assert int(a["t"][:, 0].min()) == -lim_h and int(a["t"][:, 0].max()) == lim_h and int(a["t"][:, 1].min()) == -lim_w and int(a["t"][:, 1].max()) == lim_w
    r0, r1, c0, c1 = a["rect"].unbind(1)
    assert bool(((0 <= r0) & (r0 < r1) & (r1 <= H) & (0 <= c0) & (c0 < c1) & (c1 <= W)).all())          # non-empty, inside the image
    assert int((r1 - r0).max()) == int(H * 0.5 + 0.5) and int((c1 - c0).max()) == int(W * 0.5 + 0.5)
    # the documented order of the draws, replayed
    torch.manual_seed(3)
    torch.rand([3, N])
    assert torch.equal(torch.rand([N]) - 0.5, a["b"]) and torch.equal(torch.rand([N]) * 2, a["s"]) and torch.equal(torch.rand([N]) + 0.5, a["k"])
    assert torch.equal(torch.randint(-lim_h, lim_h + 1, [N]).to(torch.int32), a["t"][:, 0])
    assert torch.equal(torch.randint(-lim_w, lim_w + 1, [N]).to(torch.int32), a["t"][:, 1])
    # a disabled group draws nothing and keeps its identity parameters
    torch.manual_seed(3)
    only_t = A.DiffAugmentPipe(translation=1).sample(N, C, H, W)
    torch.manual_seed(3)
    torch.rand([1, N])
    assert torch.equal(torch.randint(-lim_h, lim_h + 1, [N]).to(torch.int32), only_t["t"][:, 0])
    ident = D.identity_params(N)
    assert all(torch.equal(only_t[k], ident[k]) for k in ("b", "s", "k", "rect"))


def test_sampler_gates():
    pipe = A.DiffAugmentPipe(color=1, translation=1, cutout=1)
    N, C, H, W = 4096, 3, 16, 16
    ident = D.identity_params(N)
    torch.manual_seed(0)
    z = pipe.sample(N, C, H, W, p=0.0)
    assert all(torch.equal(z[k], ident[k]) and z[k].dtype == ident[k].dtype for k in ident)
    pipe.p.copy_(torch.as_tensor(0.0))                  # and through the buffer
    z = pipe.sample(N, C, H, W)
    assert all(torch.equal(z[k], ident[k]) for k in ident)
    one = pipe.sample(N, C, H, W, p=1.0)
    assert bool((one["rect"][:, 1] > one["rect"][:, 0]).all())          # p = 1: every sample gets every group (the published behaviour)
    p = 0.3
    torch.manual_seed(1)
    a = pipe.sample(N, C, H, W, p=p)
    tol = 5 * math.sqrt(p * (1 - p) / N)
    f_cut = float((a["rect"][:, 1] > a["rect"][:, 0]).float().mean())                    # an applied cutout is never empty
    f_col = float((a["k"] != 1).float().mean())                                          # k = rand + 0.5 hits 1.0 with probability 2^-24
    # an applied shift is (0, 0) once in 25 draws (lim = 2 on both axes), so the translation gate is counted through the replayed
    # gate draw itself: the first draw of a call, rand([3, N]), rows colour / translation / cutout
    torch.manual_seed(1)
    gates = torch.rand([3, N]) < p
    assert abs(f_col - p) <= tol and abs(f_cut - p) <= tol
    for g in range(3):
        assert abs(float(gates[g].float().mean()) - p) <= tol
    assert torch.equal(a["k"] != 1, gates[0]) and torch.equal(a["rect"][:, 1] > a["rect"][:, 0], gates[2])
    assert bool((a["t"][~gates[1]] == 0).all()) and bool((a["t"][gates[1]] != 0).any())


def test_cutout_rectangle_is_the_clamped_scatter():
    """exhaustive: every extent 5..8, every window size (odd and even), every offset the sampler can draw"""
    for H in range(5, 9):
        for size in range(1, H + 1):
            for o in range(0, H + (1 - size % 2)):
                cleared = sorted(set(int(v) for v in U.scatter_indices(o, size, H)))
                r0, r1 = A.DiffAugmentPipe.cutout_rect(torch.as_tensor(o), size, H)
                assert cleared == list(range(int(r0), int(r1))) and int(r1) > int(r0), (H, size, o)
    # two axes at once, through the sampler, against the scattered mask
    pipe = A.DiffAugmentPipe(cutout=1, cutout_ratio=0.5)
    torch.manual_seed(5)
    H, W, N = 7, 6, 64
    prm = pipe.sample(N, 3, H, W, p=1.0)
    torch.manual_seed(5)
    torch.rand([1, N])
    o_row, o_col = torch.randint(0, H + (1 - 4 % 2), [N]), torch.randint(0, W + (1 - 3 % 2), [N])
    for n in range(N):
        assert torch.equal(U.rect_mask(prm["rect"][n], H, W), U.scatter_mask(H, W, 4, 3, o_row[n], o_col[n]))


def _cases():
    gen = torch.Generator().manual_seed(11)
    for (N, C, H, W, tr, cr) in [(4, 3, 6, 10, 0.125, 0.5), (3, 1, 5, 7, 0.5, 0.3), (2, 4, 8, 4, 1.0, 1.0), (3, 3, 7, 5, 0.25, 0.5)]:
        prm = U.random_params(gen, N, H, W, tr, cr)
        x = torch.randn([N, C, H, W], generator=gen, dtype=torch.float64)
        g = torch.randn([N, C, H, W], generator=gen, dtype=torch.float64)
        yield x, g, prm
    # shifts of the whole extent and beyond, whole-image and empty rectangles, rectangles that leave the image
    N, C, H, W = 6, 3, 5, 6
    prm = U.make_params([0.25, -0.5, 0, 0.1, 0.2, 0.3], [0, 0.5, 1, 2, 1.5, 0.7], [0.5, 1, 1.5, 1.2, 0.9, 1],
                        [[H, 0], [0, -W], [-H - 3, 2], [2, W + 100], [0, 0], [-1, 1]],
                        [[0, 0, 0, 0], [0, H, 0, W], [-3, 2, 4, 99], [3, 1, 0, W], [1, 2, 0, W], [0, H, 2, 3]])
    yield torch.randn([N, C, H, W], generator=gen, dtype=torch.float64), torch.randn([N, C, H, W], generator=gen, dtype=torch.float64), prm


def test_reference_and_functions_match_the_published_ops_in_float64():
    worst = 0.0
    for x, g, prm in _cases():
        y_ref, dx_ref = U.published_with_adjoint(x, g, prm)
        # the published composition, op by op
        xr = x.clone().requires_grad_(True)
        y1 = D.diffaug_reference(xr, prm)
        dx1, = torch.autograd.grad((y1 * g).sum(), xr)
        # the fused form through the two Functions (packed table and dict alike)
        xf = x.clone().requires_grad_(True)
        y2 = D.diffaug(xf, D.pack(prm))
        dx2, = torch.autograd.grad((y2 * g).sum(), xf)
        y3 = D.diffaug(x, prm)
        dx3 = D.diffaug_adjoint(g, prm)
        assert y1.dtype == torch.float64 and y2.dtype == torch.float64
        for got, want in ((y1, y_ref), (dx1, dx_ref), (y2, y_ref), (dx2, dx_ref), (y3, y_ref), (dx3, dx_ref)):
            worst = max(worst, float((got.detach() - want).abs().max()))
    assert worst < 1e-13, worst                         # float64 round-off of a handful of operations on values of order 1
    # fp32 in, fp32 out
    x, g, prm = next(_cases())
    assert D.diffaug(x.float(), prm).dtype == torch.float32 and D.diffaug_reference(x.float(), prm).dtype == torch.float32


def test_identity_parameters_return_the_input_bits():
    torch.manual_seed(2)
    x = torch.randn(3, 3, 6, 5)
    y = D.diffaug(x, D.identity_params(3))
    assert torch.equal(y.view(torch.int32), x.view(torch.int32))
    pipe = A.DiffAugmentPipe(color=1, translation=1, cutout=1)
    pipe.p.copy_(torch.as_tensor(0.0))
    assert torch.equal(pipe(x).view(torch.int32), x.view(torch.int32))


def test_gradcheck_and_gradgradcheck():
    gen = torch.Generator().manual_seed(4)
    N, C, H, W = 2, 3, 4, 5
    prm = U.make_params([0.3, -0.2], [0.4, 1.7], [1.3, 0.6], [[1, -1], [0, 2]], [[1, 3, 0, 2], [0, 2, 3, 5]])
    table = D.pack(prm)
    x = torch.randn([N, C, H, W], generator=gen, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: D.diffaug(t, table), (x,))
    assert torch.autograd.gradgradcheck(lambda t: D.diffaug(t, table), (x,))
    # a nonlinear head, so that the second derivative through the pair of Functions is not trivially zero
    assert torch.autograd.gradgradcheck(lambda t: D.diffaug(t, table).square(), (x,))
    assert torch.autograd.gradcheck(lambda t: D.diffaug_adjoint(t, table), (x,))


def test_validation_names_the_op():
    x = torch.randn(2, 3, 4, 4)
    prm = D.identity_params(2)
    with pytest.raises(RuntimeError, match="diffaug"):
        D.diffaug(x[0], prm)                            # not [N, C, H, W]
    with pytest.raises(RuntimeError, match="diffaug"):
        D.diffaug(x, D.pack(D.identity_params(3)))      # table of another batch size
    with pytest.raises(RuntimeError, match="diffaug"):
        D.diffaug(x, D.pack(prm).to(torch.int64))       # wrong table dtype
    with pytest.raises(RuntimeError, match="diffaug"):
        D.diffaug(x.to(torch.int32), prm)               # integer images
    with pytest.raises(RuntimeError, match="diffaug"):
        D.diffaug(x, dict(prm, t=torch.zeros(2, 2)))    # a float shift
