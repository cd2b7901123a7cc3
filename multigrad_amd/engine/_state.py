"""Checkpoints of the fused engine: this rank's optimizer state out and back in."""
from __future__ import annotations

from typing import Optional

import torch

from ._stream import on_engine_stream


class _StateMixin:
    @property
    def sharded(self) -> bool:
        return self.size > 1 and (self.zero or self.owner)

    def _mode(self) -> str:
        return "owner" if self.owner else "zero" if self.zero else "replicated"

    def _local_theta(self) -> torch.Tensor:
        return self._local(self.theta)

    @on_engine_stream
    def state_dict(self) -> dict:
        """This rank's optimizer state after ``step_host`` steps: owned slices under ZeRO
        and owner mode (one file per rank), everything otherwise."""
        self.drain()
        self.check("state_dict")  # never checkpoint NaN-poisoned state
        st = {"mode": self._mode(), "size": self.size, "rank": self.rank, "P": self.P,
              "pb": list(self.pb), "step": self.step_host, "lr": self.lr,
              "theta": self._local_theta().detach().cpu().clone(),
              "m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
              "u": None if self.u is None else self.u.detach().cpu().clone()}
        rows = self.step_host + 1
        if self.traj_loc is not None:
            st["traj"] = self._traj_rows_to_current(self.traj_loc[:rows]).detach().cpu().clone()
        elif self.history.mode == "full":
            st["traj"] = self._traj_rows_to_current(self.history.buf[:rows]).detach().cpu().clone()
        else:
            st["history_rows"] = [r.detach().cpu().clone() for r in self.history.rows]
        if self.pidx is not None:
            # the user parameter index of every local element: a checkpoint written after a
            # re-layout loads into an engine laid out differently (e.g. at the guess)
            st["units_order"] = self._local_order().cpu().clone()
            if self.history.mode != "full" and self.traj_loc is None:
                st["units_order_full"] = self.pidx.cpu().clone()
        return st

    def _local_order(self) -> torch.Tensor:
        """User parameter index of each element of this rank's optimizer vectors (owner
        mode; the whole order otherwise: ZeRO slices are cut from it, see
        :meth:`_reorder_loaded`)."""
        return self._local(self.pidx) if self.owner else self.pidx

    @on_engine_stream
    def load_state_dict(self, st: dict) -> int:
        """Restore a :meth:`state_dict` into a :meth:`setup` engine of the same shape;
        returns the step to continue from."""
        # finish this engine's in-flight work first: a pending fused exchange (the last chunk's
        # reduce-scatter -> Adam -> all-gather, carried by the next launch) or a pending
        # pipelined update would otherwise run on top of the loaded state
        self.drain()
        mode = self._mode()
        if st["mode"] != mode or st["size"] != self.size or st["P"] != self.P or \
                list(st["pb"]) != list(self.pb):
            raise ValueError(f"checkpoint ({st['mode']}, {st['size']} ranks) does not match "
                             f"this engine ({mode}, {self.size} ranks)")
        dev = self.device
        step = int(st["step"])
        from ..utils.checkpoint import check_loaded_step
        check_loaded_step(step, self.comm if self.size > 1 else None)
        self.m.copy_(st["m"].to(dev))
        self.v.copy_(st["v"].to(dev))
        th = st["theta"].to(dev)
        for s in self.slices:
            self.theta[s.a:s.b].copy_(th[s.o:s.o + s.n])
        if self.zero and not self.owner:  # every rank's slices into every rank's theta
            for s in self.slices:
                self._all_gather(s)
            self.drain()
        if st.get("u") is not None:
            self.u.copy_(st["u"].to(dev))
        if "traj" in st:
            tr = st["traj"].to(dev)
            dst = self.traj_loc if self.traj_loc is not None else self.history.buf
            dst[:tr.shape[0]].copy_(tr)
        elif "history_rows" in st:
            self.history.rows = [r.to(dev) for r in st["history_rows"]]
        if st.get("units_order") is not None and self.pidx is not None:
            full = st.get("units_order_full")
            self._reorder_loaded(st["units_order"].to(dev), None if full is None else full.to(dev))
        self._segs = [(0, self.inv_pidx)]
        self.step_host = step
        self.step_dev[:, 0] = step
        self.step_dev[:, 1] = 0
        return step

    def _reorder_loaded(self, saved: torch.Tensor, saved_full: Optional[torch.Tensor]) -> None:
        """Permute freshly loaded vectors from the checkpoint's internal order (``saved``:
        user index per local element; ``saved_full``: per element of the full vector) into
        this engine's."""
        def positions(order):
            pos = torch.empty(self.P, dtype=torch.int64, device=order.device)
            pos[order] = torch.arange(order.numel(), device=order.device)
            return pos

        cur = self._local_order()
        if not torch.equal(saved, cur) and self.zero and not self.owner:
            # ZeRO slices are cut from the internal order: a different lanes layout gives
            # every rank different parameters in its slices
            raise ValueError(
                "this ZeRO checkpoint was written with a different lanes layout (parameter "
                "order) than this engine's -- e.g. resumed from another starting point whose "
                "narrow populations group the lanes differently; resume with the run's own "
                "guess, with zero=False, or with MULTIGRAD_LANE_CLASSES=0 on both runs")
        if not torch.equal(saved, cur):
            idx = positions(saved)[cur]  # position of each current local element when saved
            n = cur.numel()
            a = self.slices[0].a  # one slice: owner mode or replicated
            self.theta[a:a + n] = self.theta[a:a + n][idx]
            for t in (self.m, self.v, self.u):
                if t is not None:
                    t[:n] = t[:n][idx]
            traj = self.traj_loc if self.traj_loc is not None else (
                self.history.buf if self.history.mode == "full" else None)
            if traj is not None:
                traj[:, :n] = traj[:, :n][:, idx]
        if saved_full is not None and self.history.mode != "full" and self.traj_loc is None \
                and not torch.equal(saved_full, self.pidx):
            idx = positions(saved_full)[self.pidx]
            self.history.rows = [r[idx] for r in self.history.rows]

    @on_engine_stream
    def save_checkpoint(self, path: str) -> None:
        from ..utils import checkpoint as ckpt
        self.drain()
        self.check("checkpoint", collective=True)
        ckpt.save_optimizer_state(path, self.state_dict(), comm=self.comm if self.size > 1 else None,
                                  sharded=self.sharded)

    @on_engine_stream
    def load_checkpoint(self, path: str) -> int:
        from ..utils import checkpoint as ckpt
        return self.load_state_dict(ckpt.load_optimizer_state(
            path, rank=self.rank, sharded=self.sharded,
            comm=self.comm if self.size > 1 and self.sharded else None))
