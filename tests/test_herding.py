"""ops.herding_select on the CPU, and its use by FedSTIL.build_examplars."""

import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

from herding_oracle import TOL, make_groups, worst_excess


def test_cpu_entry_is_the_reference_and_float64_optimal():
    feats, pids = make_groups([1, 2, 3, 8, 33, 65], 36, seed=0)
    persons, chosen = ops.herding_select(feats, pids, 32)
    ref_persons, ref_chosen = ref.herding_select(feats, pids, 32)
    assert persons == ref_persons and torch.equal(chosen, ref_chosen)
    assert chosen.shape == (6, 32) and chosen.dtype == torch.int64
    assert worst_excess(feats, pids, persons, chosen) <= TOL
    assert ops.herding_route(65, 36, torch.float32, False) == "torch"


def test_fedstil_build_examplars_goes_through_the_entry(monkeypatch):
    from flreid_amd.runtime.builder import parser_model
    model = parser_model("fedstil", {
        "name": "resnet18", "num_classes": 64, "last_stride": 1,
        "neck": "bnneck", "fine_tuning": ["classifier"],
        "atten_default": 0.9, "lambda_k": 8})
    model.ids.update([3, 9, 11])                   # m = ceil(8 / 3) = 3
    monkeypatch.setattr(model, "head_forward", lambda x: x.flatten(1))
    monkeypatch.setattr(model, "eval_graphed",
                        lambda name, fn, data, full: fn(data))
    calls = []
    entry = ops.herding_select

    def recording(feats, pids, m, route=None):
        calls.append((tuple(feats.shape), pids.tolist(), m, route))
        return entry(feats, pids, m, route=route)

    monkeypatch.setattr(ops, "herding_select", recording)
    pids = torch.tensor([9, 3, 11, 9, 3, 9, 11, 9])
    loader = [(torch.randn(4, 2, 3, 2), pids[:4], pids[:4] % 4),
              (torch.randn(4, 2, 3, 2), pids[4:], pids[4:] % 4)]
    # the rehearsal set steers training: the reference selection unless the
    # kernel is asked for
    monkeypatch.delenv("FLREID_HERDING", raising=False)
    model.build_examplars(loader, None, "cpu")
    monkeypatch.setenv("FLREID_HERDING", "kernel")
    model.build_examplars(loader, None, "cpu")
    assert calls == [((8, 12), pids.tolist(), 3, "torch"),
                     ((8, 12), pids.tolist(), 3, None)]
    assert sorted(model.examplars) == [3, 9, 11]
    for pid, (protos, classes) in model.examplars.items():
        assert protos.shape == (3, 2, 3, 2) and classes.tolist() == [pid % 4] * 3
