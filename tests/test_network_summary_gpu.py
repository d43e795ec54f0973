"""The network summary tool on the device, on the sg2_classic networks of `test_calc_metrics_cpu.SG2_YAML` at 16 x 16 with two reduced-precision
resolutions: every entry's running records equal act_stats' CPU path applied to the same captured tensors, bit for bit; the dtype and memory
format columns show the 16-bit channel-minor and the fp32 contiguous entries; the files do not depend on --batch."""
import json
import os

import numpy as np
import pytest
import torch

import act_stats_util as U
from test_calc_metrics_cpu import _run
from style_big_gan_amd import arguments, network_summary as NS, tool_support
from style_big_gan_amd.torch_utils.ops import act_stats as A

pytestmark = pytest.mark.gpu

LOW = ["gens_args.sg2_classic.synthesis_kwargs.num_fp16_res=2", "discs_args.sg2_classic.num_fp16_res=2"]


@pytest.fixture(scope="module")
def networks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("network_summary_gpu")
    trainer, overrides, _, data = _run(tmp)
    snap = str(tmp / "snaps" / "network-snapshot-000001.pt")
    state = trainer.engine.G_ema if trainer.engine.G_ema is not None else trainer.engine.G
    torch.save({"G_ema": {k: v.detach().cpu() for k, v in state.state_dict().items()},
                "D": {k: v.detach().cpu() for k, v in trainer.engine.D.state_dict().items()}}, snap)
    return overrides + LOW, snap, data, tmp


def test_records_equal_the_cpu_path_on_the_captured_tensors(networks):
    overrides, snap, data, tmp = networks
    config = arguments.load_config(overrides)
    dev = torch.device("cuda", torch.cuda.current_device())
    G = tool_support.load_generator(config, snap, dev, announce=False)
    D = tool_support.load_discriminator(config, snap, G, dev)
    captured = {}

    def on_output(key, name, t):
        host = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype)          # the same layout on the host
        host.copy_(t)
        captured.setdefault((key, name), []).append(host)

    with tool_support.open_dataset(config, tool_support.dataset_kwargs_for(config, G, data=data, mirror=False)) as dataset:
        result = NS.measure_networks(G, D=D, seeds=range(10), dataset=dataset, batch=4, device=dev, on_output=on_output)
    assert list(result["report"]) == ["G", "D(fake)", "D(real)"] and len(captured) > 20
    arrays = result["arrays"]
    for (key, name), tensors in captured.items():
        found = [k for k in arrays if k.startswith(key + ".") and k.endswith("." + name + ".counts")]
        assert len(found) == 1, (key, name, found)
        assert [t.shape[0] for t in tensors] == [4, 4, 2]
        rc, rv = A.empty(tensors[0].shape[1])
        for t in tensors:
            A.fold(*A.planes(t), rc, rv)
        assert U.same_bits(arrays[found[0]], rc.numpy()), (key, name, U.first_difference(arrays[found[0]], rc.numpy()))
        values = arrays[found[0].replace(".counts", ".values")]
        assert U.same_bits(values, rv.numpy()), (key, name, U.first_difference(values, rv.numpy()))
    rows = [e for net in result["report"].values() for e in net["entries"] if e["stats"] is not None]
    assert any(e["dtype"] in ("bfloat16", "float16") and e["memory_format"] == "channels_last" for e in rows)
    assert any(e["dtype"] == "float32" and e["memory_format"] == "contiguous" for e in rows)
    for key in ("G", "D(fake)", "D(real)"):
        assert result["report"][key]["first_nonfinite"] is None and result["report"][key]["samples"] == 10
    for key, net in (("G", G), ("D(fake)", D)):
        assert result["report"][key]["parameters"] == sum(p.numel() for p in net.parameters())


def test_the_cli_writes_the_files_whatever_the_batch(networks):
    overrides, snap, data, tmp = networks
    outs = []
    for batch in (3, 8):
        out = str(tmp / f"out{batch}")
        NS.run_network_summary(overrides + [f"--snapshot={snap}", f"--outdir={out}", f"--data={data}", "--seeds=0-7", f"--batch={batch}", "--device=cuda"])
        assert sorted(os.listdir(out)) == ["exponents.png", "summary.json", "summary.npz", "summary.txt"]
        json.loads(open(os.path.join(out, "summary.json")).read(), parse_constant=lambda token: pytest.fail(f"not strict JSON: {token}"))
        outs.append(np.load(os.path.join(out, "summary.npz")))
    a, b = outs
    assert a.files == b.files
    differing = [k for k in a.files if not U.same_bits(a[k], b[k])]
    # D's minibatch standard deviation mixes the samples of a group of 4, so the entries from it on depend on the batching; all others may not
    assert all(k.startswith("D(") for k in differing), differing
    g_keys = [k for k in a.files if k.startswith("G.")]
    assert g_keys and not [k for k in differing if k in g_keys]
