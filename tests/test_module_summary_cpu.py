"""torch_utils/misc.py `print_module_summary` / `module_summary`: the printed text equals, character for character, what the reference's own
function printed for the same toy modules (tests/golden/module_summary_*.txt, recorded by tests/golden/make_module_summary_golden.py), and the
totals equal the parameter counts of the package's cnn32_dcgan networks."""
import contextlib
import io
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd.torch_utils import misc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


class Leaf(torch.nn.Module):
    """a parameter and a buffer"""

    def __init__(self, features):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(features, features))
        self.register_buffer("offset", torch.zeros(features))

    def forward(self, x):
        return x @ self.weight + self.offset


class Pair(torch.nn.Module):
    """returns a tuple of two tensors of different shapes and dtypes, and something that is no tensor"""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(1))

    def forward(self, x):
        return x * self.scale, x[:, :2].to(torch.float64), "text"


class Tied(torch.nn.Module):
    """uses a parameter another module owns"""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight

    def forward(self, x):
        return x @ self.weight.t()


class PassThrough(torch.nn.Module):
    """no parameter, and its output is the tensor it was given: redundant"""

    def forward(self, x):
        return x


class Level(torch.nn.Module):
    """one level of nesting around `inner`"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return torch.relu(self.inner(x))


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.first = Leaf(4)
        self.tied = Tied(self.first.weight)
        self.same = PassThrough()
        self.deep = Level(Level(Level(Level(Leaf(4)))))         # deep.inner.inner.inner.inner: nesting 5
        self.pair = Pair()
        self.register_buffer("count", torch.zeros(3, dtype=torch.int64))

    def forward(self, x, y):
        x = self.same(self.tied(self.first(x)))
        a, b, _ = self.pair(self.deep(x) + y)
        return a, b


def _toy():
    torch.manual_seed(0)
    return Toy(), [torch.ones(2, 4), torch.zeros(2, 4)]


def _sequential():
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 1)), [torch.ones(7, 3)]


# name -> (module and inputs, the keyword arguments): the golden files carry these names
CASES = {
    "toy": (_toy, dict()),
    "toy_keep_redundant": (_toy, dict(skip_redundant=False)),
    "toy_nesting1": (_toy, dict(max_nesting=1)),
    "toy_nesting9": (_toy, dict(max_nesting=9, skip_redundant=False)),
    "sequential": (_sequential, dict()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_text_is_the_reference_s(name):
    make, kwargs = CASES[name]
    module, inputs = make()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        outputs = misc.print_module_summary(module, inputs, **kwargs)
    with open(os.path.join(GOLDEN, f"module_summary_{name}.txt")) as fh:
        want = fh.read()
    assert text.getvalue() == want
    again = module(*inputs)
    if isinstance(outputs, tuple):
        assert len(outputs) == len(again) and all(torch.equal(a, b) for a, b in zip(outputs, again))
    else:
        assert torch.equal(outputs, again)
    assert not any(m._forward_hooks or m._forward_pre_hooks for m in module.modules())           # the hooks are gone


def test_what_the_toy_cases_cover():
    module, inputs = _toy()
    entries, _ = misc.module_summary(module, inputs)
    names = [e.name for e in entries]
    assert "same" not in names and "deep.inner.inner.inner" not in names and "deep.inner.inner" in names and names[-1] == "<top-level>"
    by_name = {e.name: e for e in entries}
    assert by_name["first"].params == 16 and by_name["first"].buffers == 4 and by_name["tied"].params == 0       # the shared weight is counted once
    assert by_name["pair"].labels() == ["pair:0", "pair:1"] and [tuple(t.shape) for t in by_name["pair"].outputs] == [(2, 4), (2, 2)]
    assert by_name["<top-level>"].buffers == 3 and by_name["<top-level>"].new_outputs == []
    kept, _ = misc.module_summary(module, inputs, skip_redundant=False)
    assert "same" in [e.name for e in kept] and [e for e in kept if e.name == "same"][0].redundant
    assert sum(e.params for e in entries) == sum(p.numel() for p in module.parameters()) == 16 + 16 + 1
    assert sum(e.buffers for e in entries) == sum(b.numel() for b in module.buffers())
    with pytest.raises(TypeError):
        misc.module_summary(module, inputs[0])


def test_totals_of_the_package_s_dcgan_networks():
    from style_big_gan_amd.train_parts.discriminators import discriminators
    from style_big_gan_amd.train_parts.generators import generators
    G = generators["cnn32_dcgan"](z_dim=100, c_dim=0, img_resolution=32).eval()
    D = discriminators["cnn32_dcgan"]().eval()
    with torch.no_grad():
        g_entries, img = misc.module_summary(G, [torch.zeros(2, 100), None])
        d_entries, logits = misc.module_summary(D, [img, None])
    assert tuple(img.shape) == (2, 3, 32, 32) and tuple(logits.shape) == (2, 1)
    for net, entries in ((G, g_entries), (D, d_entries)):
        assert sum(e.params for e in entries) == sum(p.numel() for p in net.parameters())
        assert sum(e.buffers for e in entries) == sum(b.numel() for b in net.buffers())
        assert "<top-level>" not in [e.name for e in entries]          # it returns its last layer's tensor and owns nothing itself: redundant
