"""Resume bookkeeping on the host (no GPU, no launch): what FlatAdamW rebuilds from a stock torch.optim.AdamW state dict, the
dropout position accessor, and the record comparison of tests/resume_cases.py itself.  (arena.FlatAdam refuses CPU
parameters at construction: its bookkeeping after a load is asserted in tests/test_gpu_resume.py, in every record.)"""
import pytest
import torch

import resume_cases as rc


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _stock_state(m, steps):
    stock = torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=0.02)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g) * 1e-2
        stock.step()
    return stock


@pytest.mark.parametrize("BN", [True, False])
def test_flat_adamw_bookkeeping_after_loading_a_stock_state(pkg, BN):
    torch.manual_seed(0)
    m = pkg.LinearModel(34, 51, linear_size=64, num_stage=1, p_dropout=0.5, BN=BN)
    sd = _stock_state(m, 7).state_dict()
    assert float(sd["state"][0]["step"]) == 7.0
    opt = pkg.FlatAdamW(m, lr=1e-3)
    opt.load_state_dict(sd)
    assert opt._t == 7 and opt.skipped_steps() == 0
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["weight_decay"] == 0.02
    flat = m.flat_params
    assert opt._m.shape == flat.shape and opt._v.shape == flat.shape
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for k, (s, p) in enumerate(zip(m._slots, m._param_list)):
        st = opt.state[p]
        assert st["step"] is opt._step_tensor and float(st["step"]) == 7.0
        # views of the arenas at the slot's offset, holding the loaded values
        assert st["exp_avg"].data_ptr() == opt._m.data_ptr() + 4 * s.offset and st["exp_avg"].shape == p.shape
        assert st["exp_avg_sq"].data_ptr() == opt._v.data_ptr() + 4 * s.offset
        assert p.data_ptr() == flat.data_ptr() + 4 * s.offset
        assert torch.equal(st["exp_avg"], sd["state"][k]["exp_avg"]) and bool(st["exp_avg"].any())
        assert torch.equal(st["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
        assert torch.equal(opt._m[s.offset:s.offset + s.numel].view(s.shape), sd["state"][k]["exp_avg"])
        covered[s.offset:s.offset + s.numel] = True
    assert not bool(opt._m[~covered].any()) and not bool(opt._v[~covered].any())      # alignment padding stays zero
    back = opt.state_dict()
    assert len(back["state"]) == len(sd["state"]) == len(m._slots)
    for k in sd["state"]:
        assert float(back["state"][k]["step"]) == 7.0
        assert torch.equal(back["state"][k]["exp_avg"], sd["state"][k]["exp_avg"])
        assert torch.equal(back["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
    # and a second load (a lower count) replaces the first: the count is not a running maximum across loads
    opt.load_state_dict(_stock_state(m, 2).state_dict())
    assert opt._t == 2 and float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_dropout_state_is_what_manual_seed_takes_and_stays_out_of_state_dict(pkg):
    torch.manual_seed(5)
    m = pkg.LinearModel(34, 51, linear_size=64, num_stage=1)
    assert m.dropout_state() == {"seed": 5, "step": 0}
    m.manual_seed(0xFEDCBA9876543210, step=41)
    st = m.dropout_state()
    assert st == {"seed": 0xFEDCBA9876543210, "step": 41} and all(type(v) is int for v in st.values())
    other = pkg.LinearModel(34, 51, linear_size=64, num_stage=1)
    assert other.manual_seed(**st) is other and other.dropout_state() == st
    keys = set(m.state_dict())
    assert not any("seed" in k or "dropout" in k or k.endswith("step") for k in keys)
    # the reference's key set: Linear / BatchNorm1d entries only
    assert all(k.rsplit(".", 1)[1] in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked") for k in keys)


def test_record_comparison_sees_one_ulp():
    a = dict(loss=torch.tensor(1.0), params=torch.ones(8), exp_avg=[torch.zeros(3)], exp_avg_sq=[torch.zeros(3)],
             bn=[torch.ones(2)], step=4.0, lr=1e-3, y_hat=None)
    b = {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v] if isinstance(v, list) else v) for k, v in a.items()}
    rc.assert_same(a, b)
    b["params"][5] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0))
    assert rc.differs(a, b)
    b["params"][5] = 1.0
    b["step"] = 3.0
    assert rc.differs(a, b)
    b["step"] = 4.0
    b["exp_avg"][0][1] = 1e-30
    assert rc.differs(a, b)
