"""il_checkpoint without a GPU: BestAgentSaver's write schedule against the list the reference's own class wrote
(tests/golden/best_agent_saver.json, made by tests/golden/gen_best_agent_saver.py), the file format's round trip, and its
refusals.  The agents here are CPU stand-ins with the state_dict / load_state_dict contract; the device objects are in
tests/test_gpu_il_checkpoint.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from olympic_hip import il_checkpoint as ck
from olympic_hip._ffi import OlyError
from olympic_hip.gail import _same

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "best_agent_saver.json")
CASES = json.load(open(FIXTURE))["cases"]


class EpochAgent:
    """An agent whose state changes every epoch: the tensor holds the epoch, written in place as a device agent's
    parameters are, so a snapshot that kept a reference instead of a clone would show the latest epoch."""

    def __init__(self, kind="vail", dim=3):
        self.kind, self.dim = kind, dim
        self.w = torch.zeros(dim, dtype=torch.float64)
        self.iter = 0

    def set_epoch(self, e):
        self.w.fill_(float(e))
        self.iter = int(e)

    def state_dict(self):
        return dict(header=dict(kind=self.kind, in_dim=self.dim), iter=self.iter, w=self.w.clone())

    def load_state_dict(self, d):
        _same("EpochAgent", "kind", d["header"]["kind"], self.kind)
        _same("EpochAgent", "in_dim", d["header"]["in_dim"], self.dim)
        self.w.copy_(d["w"])
        self.iter = int(d["iter"])


# ------------------------------------------------------------------------------ the saver against the reference's list
def test_the_fixture_holds_what_the_issue_lists():
    got = {(c["sequence"], c["n_epochs_save"]): [w["epoch"] for w in c["writes"]] for c in CASES}
    assert got[("issue", 1)] == [0, 2, 3, 4, 5, 6, 7]        # not 1: the write lags the snapshot by one call
    assert got[("issue", 3)] == [2, 5, 7]
    assert got[("issue", -1)] == []
    assert got[("issue", 500)] == [5]
    assert {c["n_epochs_save"] for c in CASES} == {1, 3, -1, 500} and len({c["sequence"] for c in CASES}) >= 2
    seq = [c["J"] for c in CASES if c["sequence"] == "issue"][0]
    assert seq == [1, .5, 2, 2, 1.5, 3, -1, 0]
    for c in CASES:                                          # a decrease and a negative J in every sequence, a tie in two
        J = c["J"]
        assert any(b < a for a, b in zip(J, J[1:])) and min(J) < 0
    assert sum(any(a == b for a, b in zip(c["J"], c["J"][1:])) for c in CASES if c["n_epochs_save"] == 1) >= 2


@pytest.mark.parametrize("case", CASES, ids=[f"{c['sequence']}-{c['n_epochs_save']}" for c in CASES])
def test_saver_writes_what_the_reference_writes(case, tmp_path):
    saver = ck.BestAgentSaver(str(tmp_path), n_epochs_save=case["n_epochs_save"])
    agent = EpochAgent()
    writes = []
    for call, J in enumerate(case["J"]):
        agent.set_epoch(call)
        before = set(os.listdir(tmp_path))
        path = saver.save(agent, J)
        new = sorted(set(os.listdir(tmp_path)) - before)
        assert new == ([] if path is None else [os.path.basename(path)])
        writes += [(n, call) for n in new]
    agent.set_epoch(len(case["J"]))                          # the agent moves on before the final write
    before = set(os.listdir(tmp_path))
    path = saver.save_curr_best_agent()
    new = sorted(set(os.listdir(tmp_path)) - before)
    assert new == ([] if path is None else [os.path.basename(path)])
    writes += [(n, len(case["J"])) for n in new]
    assert saver.save_curr_best_agent() is None              # forgotten after the write
    assert [(w["stem"] + ".pt", w["call"]) for w in case["writes"]] == writes
    assert sorted(os.listdir(tmp_path)) == sorted(w["stem"] + ".pt" for w in case["writes"])   # no .part left behind
    for w in case["writes"]:                                 # each file holds the state of its own epoch
        other = EpochAgent()
        meta = ck.load(str(tmp_path / (w["stem"] + ".pt")), other)
        assert meta == dict(epoch=w["epoch"], J=w["J"])
        assert other.iter == w["epoch"] and torch.equal(other.w, torch.full((3,), float(w["epoch"]), dtype=torch.float64))
        assert w["stem"] == "agent_epoch_%d_J_%f" % (w["epoch"], w["J"])


def test_save_agent_writes_at_once(tmp_path):
    saver = ck.BestAgentSaver(str(tmp_path / "sub"), n_epochs_save=-1)
    agent = EpochAgent()
    agent.set_epoch(4)
    path = saver.save_agent(agent, -0.25)
    assert os.path.basename(path) == "agent_J_-0.250000.pt" and os.listdir(tmp_path / "sub") == ["agent_J_-0.250000.pt"]
    other = EpochAgent()
    assert ck.load(path, other) == dict(J=-0.25) and other.iter == 4


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree exists in the build container only")
def test_fixture_regenerates_byte_for_byte(tmp_path):
    out = tmp_path / "again.json"
    env = dict(os.environ, PYTHONHASHSEED="random")
    for k in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS"):       # the generator touches no native code
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "gen_best_agent_saver.py"), "--out", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == open(FIXTURE, "rb").read()


# ------------------------------------------------------------------------------ the format
class Nest:
    """Agent and core stand-ins holding an arbitrary nest."""

    def __init__(self, state=None):
        self.state, self.loaded = state, None

    def state_dict(self):
        return self.state

    def load_state_dict(self, d):
        self.loaded = d


def _nest(seed):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    rng.integers(0, 9, 5)
    return dict(header=dict(kind="gail", in_dim=36, pair=None, state_mask=list(range(34)), gamma=0.99),
                colstats=torch.randn((3, 36), dtype=torch.float64, generator=g), fresh=False, step=7,
                theta=torch.randn(1000, generator=g), flags=torch.randint(0, 2, (9,), generator=g).bool(),
                idx=torch.randint(-5, 5, (4, 2), generator=g, dtype=torch.int32), name="x", none=None, beta=0.1 + 1e-17,
                params=[torch.randn((4, 3), generator=g), torch.randn(4, generator=g)],
                rng=rng.bit_generator.state, gen=g.get_state(), empty={}, drawn=dict(step=dict(block=torch.zeros((2, 3),
                dtype=torch.int32), cursor=1)))


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and \
            a.numpy().tobytes() == b.numpy().tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_round_trip_is_bit_equal(tmp_path):
    agent, core = Nest(_nest(1)), Nest(_nest(2))
    path = ck.save(str(tmp_path / "a" / "b.pt"), agent, core, epoch=3, J=-1.5, note="n")
    assert path == str(tmp_path / "a" / "b.pt") and os.listdir(tmp_path / "a") == ["b.pt"]
    a2, c2 = Nest(), Nest()
    assert ck.load(path, a2, c2) == dict(epoch=3, J=-1.5, note="n")
    assert _equal(a2.loaded, _nest(1)) and _equal(c2.loaded, _nest(2))
    assert not _equal(a2.loaded, _nest(2))                   # the comparison can fail
    # the numpy generator continues from the stored state
    rng = np.random.default_rng(0)
    rng.bit_generator.state = a2.loaded["rng"]
    want = np.random.default_rng(1)
    want.integers(0, 9, 5)
    assert np.array_equal(rng.integers(0, 1 << 62, 8), want.integers(0, 1 << 62, 8))
    raw = ck.read(path)
    assert raw["format"] == "olympic_hip.il_checkpoint" and raw["version"] == 1 and set(raw) == {
        "format", "version", "agent", "core", "meta"}
    # an agent alone; asking such a file for a core is refused
    p2 = ck.save(str(tmp_path / "agent_only.pt"), agent)
    assert ck.read(p2)["core"] is None and ck.load(p2, Nest()) == {}
    with pytest.raises(OlyError, match="no core state"):
        ck.load(p2, Nest(), Nest())


def test_a_state_that_holds_an_object_is_refused_at_save(tmp_path):
    with pytest.raises(OlyError, match="ndarray"):
        ck.save(str(tmp_path / "x.pt"), Nest(dict(a=np.zeros(3))))
    assert os.listdir(tmp_path) == []


# ------------------------------------------------------------------------------ the refusals
def _file(tmp_path, **over):
    obj = dict(format=ck.FORMAT, version=ck.VERSION, agent=EpochAgent().state_dict(), core=None, meta={})
    obj.update(over)
    path = str(tmp_path / "f.pt")
    torch.save(obj, path)
    return path


def test_wrong_format_version_kind_and_dimension_name_the_field(tmp_path):
    with pytest.raises(OlyError, match=r"format is 'somebody.else', expected 'olympic_hip.il_checkpoint'"):
        ck.load(_file(tmp_path, format="somebody.else"), EpochAgent())
    with pytest.raises(OlyError, match=r"version is 2, this reader takes 1"):
        ck.load(_file(tmp_path, version=2), EpochAgent())
    torch.save([1, 2], str(tmp_path / "l.pt"))
    with pytest.raises(OlyError, match="format is 'list'"):
        ck.load(str(tmp_path / "l.pt"), EpochAgent())
    path = _file(tmp_path)
    with pytest.raises(OlyError, match=r"kind is 'vail' in the stored state, 'gail' in this object"):
        ck.load(path, EpochAgent(kind="gail"))
    with pytest.raises(OlyError, match=r"in_dim is 3 in the stored state, 5 in this object"):
        ck.load(path, EpochAgent(dim=5))
    ok = EpochAgent()
    assert ck.load(path, ok) == {}


def test_the_agents_header_check_names_the_field():
    """VAILAgent.load_state_dict's structural check on a stand-in carrying a header: nothing is written on a mismatch."""
    from olympic_hip.il_agent import GAILAgent, VAILAgent
    header = dict(kind="vail", in_dim=36, out_dim=11, disc_in_dim=34, pair=None, state_mask=list(range(34)))

    def bare(cls, **over):
        a = cls.__new__(cls)
        a._header = lambda: dict(header, kind="gail" if cls is GAILAgent else "vail", **over)
        a.policy_step, a.iter = None, 5
        return a
    stored = dict(header=dict(header), iter=9)
    for cls, over, msg in ((GAILAgent, {}, r"GAILAgent.load_state_dict: kind is 'vail' in the stored state, 'gail'"),
                           (VAILAgent, dict(in_dim=37), r"in_dim is 36 in the stored state, 37"),
                           (VAILAgent, dict(out_dim=12), r"out_dim is 11 in the stored state, 12"),
                           (VAILAgent, dict(disc_in_dim=68), r"disc_in_dim is 34 in the stored state, 68"),
                           (VAILAgent, dict(pair="next_state"), r"pair is None in the stored state, 'next_state'"),
                           (VAILAgent, dict(state_mask=list(range(33))), r"state_mask is \[0, 1, .*\] in the stored")):
        a = bare(cls, **over)
        with pytest.raises(OlyError, match=msg):
            a.load_state_dict(stored)
        assert a.iter == 5


class Local:
    pass


def test_a_file_that_needs_an_unpickled_object_is_refused(tmp_path):
    for i, obj in enumerate((Local(), dict(format=ck.FORMAT, version=ck.VERSION, agent=Local(), core=None, meta={}))):
        path = str(tmp_path / f"o{i}.pt")
        torch.save(obj, path)
        with pytest.raises(OlyError, match="unpickle an object, which is refused"):
            ck.load(path, EpochAgent())
