"""What a rank updates (``FusedAdamEngine.slices``) in every placement, and the engines'
settings parser -- setup only, on stand-ins for the communicator and the model (CPU)."""
import pytest
import torch

from multigrad_amd.engine import _env
from multigrad_amd.engine.fused import FusedAdamEngine, _Slice, plan_chunks


class _Comm:
    """One rank's view of a ``size``-rank communicator whose peers agree with it."""

    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def all_reduce(self, t, op="sum"):
        return t

    def barrier(self):
        pass

    def split(self, color):
        return self


class _Model:
    """The part of the engine protocol a setup uses; ``owner_units``: owner placement."""

    def __init__(self, J, upp, comm, owner_units=None):
        self.J, self.upp, self.comm, self.owner_units = J, upp, comm, owner_units

    def param_device(self):
        return torch.device("cpu")

    def engine_units(self):
        return self.J, self.upp

    def engine_set_chunks(self, ub):
        self.ub = list(ub)

    def engine_nS(self):
        return 4

    def engine_fwd_rows(self, chunk):
        return 1

    def engine_owner_units(self):
        return self.owner_units

    def engine_support_units(self):
        return self.owner_units[self.comm.rank], self.owner_units[self.comm.rank + 1]


def _engine(J, upp, rank, world, owner_units=None, history="full", **kw):
    comm = _Comm(rank, world) if world > 1 else None
    eng = FusedAdamEngine(_Model(J, upp, comm, owner_units), **kw)
    return eng.setup(torch.zeros(J * upp), nsteps=2, history=history)


def _once(slices_of_ranks, n):
    cover = torch.zeros(n, dtype=torch.int64)
    for slices in slices_of_ranks:
        for s in slices:
            cover[s.a:s.b] += 1
    return bool((cover == 1).all())


@pytest.mark.parametrize("J,upp,world,chunks", [(7, 2, 1, 1), (7, 2, 3, 2), (64, 2, 2, 4),
                                                (5, 2, 4, 4)])
def test_zero_slices_tile_the_planned_chunks(J, upp, world, chunks):
    ub, pb, P_pad, lengths = plan_chunks(J, upp, world, chunks)
    per_rank = []
    for rank in range(world):
        eng = _engine(J, upp, rank, world, zero=True, chunks=chunks, owner=False)
        assert eng.zero == (world > 1) and not eng.owner and eng.P_pad == P_pad
        assert len(eng.slices) == eng.C == len(lengths)
        o = 0
        for c, s in enumerate(eng.slices):
            n = lengths[c] // world
            assert (s.a, s.b, s.o, s.n, s.step) == (pb[c] + rank * n, pb[c] + (rank + 1) * n, o, n, c)
            assert s.chunk == (c if world > 1 else None)
            o += n
        assert eng.m.numel() == eng.v.numel() == o
        per_rank.append(eng.slices)
    assert _once(per_rank, P_pad)


@pytest.mark.parametrize("J,upp,ub", [(7, 2, [0, 3, 7]), (9, 2, [0, 2, 2, 9])])
def test_owner_slice_is_the_ranks_range(J, upp, ub):
    world = len(ub) - 1
    per_rank = []
    for rank in range(world):
        eng = _engine(J, upp, rank, world, owner_units=ub)
        assert eng.owner and eng.P_pad == eng.P == J * upp
        a, b = ub[rank] * upp, ub[rank + 1] * upp
        assert eng.slices == (_Slice(rank, a, b, 0, b - a, 0),)
        assert eng.m.numel() == b - a and eng.traj_loc.shape == (3, b - a)
        per_rank.append(eng.slices)
    assert _once(per_rank, J * upp)


@pytest.mark.parametrize("J,chunks,world,padded", [(8, 1, 1, False), (7, 3, 1, True),
                                                   (7, 3, 2, True)])
@pytest.mark.parametrize("history", ["full", "last"])
def test_replicated_slice_is_the_padded_vector(J, chunks, world, padded, history):
    eng = _engine(J, 2, 0, world, history=history, zero=False, chunks=chunks, owner=False)
    P, P_pad = 2 * J, plan_chunks(J, 2, 1, chunks)[2]
    assert (P_pad != P) == padded and (eng.P, eng.P_pad) == (P, P_pad)
    assert not eng.zero and not eng.owner and eng.C == chunks
    s, = eng.slices
    assert s == _Slice(None, 0, P_pad, 0, P_pad, 0)
    assert eng.m.numel() == P_pad and eng.traj_loc is None and eng.u is None
    # trajectory rows are P long: with a full trajectory the update covers [0, P) only
    args = eng._adam_args(s, 0)
    assert args["u"].numel() == args["m"].numel() == (P if history == "full" else P_pad)
    assert args["u"].data_ptr() == eng.theta.data_ptr() and args["p"] is None
    assert args["traj_stride"] == (P if history == "full" else 0)


def test_env_parser(monkeypatch):
    name = "MULTIGRAD_TEST_SETTING"
    monkeypatch.delenv(name, raising=False)
    assert _env.env_flag(name) is None and _env.env_flag(name, True) is True
    assert _env.env_int(name, 7) == 7 and _env.env_float(name, 0.5) == 0.5
    assert _env.env_choice(name, "auto", ("auto", "on", "off")) == "auto"
    for word in ("0", "false", "off", "no", " OFF ", "False", "No"):
        monkeypatch.setenv(name, word)
        assert _env.env_flag(name, True) is False
        assert _env.env_choice(name, "auto", ("auto", "on", "off")) == "off"
    for word in ("1", "true", "on", "yes", " ON ", "True", "Yes"):
        monkeypatch.setenv(name, word)
        assert _env.env_flag(name, False) is True
        assert _env.env_choice(name, "auto", ("auto", "on", "off")) == "on"
    monkeypatch.setenv(name, " 12 ")
    assert _env.env_int(name, 7) == 12 and _env.env_float(name, 0.5) == 12.0
    monkeypatch.setenv(name, "RCCL")
    assert _env.env_choice(name, "auto", ("auto", "twoshot", "rccl")) == "rccl"
    monkeypatch.setenv(name, "sideways")  # an unknown word: the default
    assert _env.env_choice(name, "auto", ("auto", "twoshot", "rccl")) == "auto"
    assert _env.env_flag(name, True) is True and _env.env_flag(name) is None


def test_settings_are_read_at_every_setup(monkeypatch):
    monkeypatch.setenv("MULTIGRAD_RELAYOUT_EVERY", "4")
    monkeypatch.setenv("MULTIGRAD_GRAPH_STEPS", "8")
    eng = FusedAdamEngine(_Model(8, 2, None))
    guess = torch.zeros(16)
    eng.setup(guess, nsteps=2)
    assert eng.relayout_every == eng.cfg.relayout_every == 4 and eng.graph_steps == 8
    monkeypatch.setenv("MULTIGRAD_RELAYOUT_EVERY", "9")
    monkeypatch.setenv("MULTIGRAD_TWOSHOT_BLOCKS", "64")
    monkeypatch.setenv("MULTIGRAD_GRAPH_STEPS", "2")  # read when the engine is constructed
    eng.setup(guess, nsteps=2)
    assert eng.relayout_every == eng.cfg.relayout_every == 9 and eng.ts_blocks == 64
    assert eng.graph_steps == eng.cfg.graph_steps == 8
