"""The batched QP as a differentiable torch layer: forward = one step on the device (QpalmBatch.step_device, after update_Q_A_device when Q / A values
are given), backward = the adjoint of the solved batch (QpalmBatch.adjoint_device).  This file only passes tensors through: the solve and the gradients
are the HIP kernels behind include/qpalm_gfx950.h.

    layer = QPLayer(batch)                       # a set-up QpalmBatch; its patterns, sizes and settings stay
    x, y, status = layer(q, bmin, bmax)          # [B][n], [B][m] float64 tensors on the batch's device (None = unchanged), optionally Qx=, Ax=
    loss(x, y).backward()                        # q.grad, bmin.grad, bmax.grad (Qx.grad, Ax.grad)

The gradient is that of the active set at the solution; members that did not end SOLVED / DUAL_TERMINATED, or whose adjoint solve
was flagged, get zero gradients -- `layer.last_adjoint` keeps the flags, residuals and pass counts of the latest backward call.

Forward-mode AD (torch.autograd.forward_ad) goes through the tangent of the solved batch (QpalmBatch.tangent_device): one direction
per forward pass, `layer.last_tangent` keeps its flags, residuals and pass counts.

backward() differentiates the state the batch holds, so it must run before the batch is solved, warm-started or updated again (by this layer or directly):
the batch counts those calls (`QpalmBatch.epoch`) and a backward() that comes too late raises RuntimeError instead of returning another solve's gradients
(the same check guards the forward-mode tangent).

QPLayer(batch, polish=True) polishes after every forward solve (QpalmBatch.polish_device with store): the x, y it returns and the
point backward() and jvp differentiate at are then the exact solution at the active set for every member whose polish was accepted (the others keep the
solve's solution); `layer.last_polish` keeps the flags, the residuals before and after, and the pass counts.

layer(q, ..., select=s) with s a [B] int64 tensor of 0 / 1 steps only the members with 1 (QpalmBatch.step_device(select=s)).  x, y and
status are still those of every member: the rows of the others are their stored solutions and statuses from before.  backward and jvp pass the same
select on, so those members cost nothing there and get zero gradients and tangents; with polish=True only the selected members are polished.  The rows of
`last_adjoint`, `last_tangent` and `last_polish` (flag, resid, passes, res) mean something for the selected members only; the others read zero.  Input rows
of members that are not selected are not read at all.  A subset forward needs every output row it returns to exist, so call it after a full forward or solve.

QPLayer(batch, replay=True) lifts the "backward before the next solve" rule: every forward also records its point -- x, y, the
active set (QpalmBatch.active_device, or the polish's own with polish=True) and the statuses -- and backward() differentiates at that record
(QpalmBatch.adjoint_device(at=...)) instead of at whatever the batch holds by then.  One batch can so be stepped T times, each q / bounds computed from the
solution before, and one backward() goes through the whole rollout.  The record is valid as long as the values of Q and A are those of its solve:
backward() raises RuntimeError only if `QpalmBatch.matrix_epoch` moved (update_Q_A*, in this layer through Qx= / Ax=).  Members whose recorded status was
not SOLVED / DUAL_TERMINATED get zero gradients, as without replay.  Forward mode (jvp) runs inside the forward pass and is the same with and without."""
import torch

from .solver import SOLVED, DUAL_TERMINATED


class _QPFunction(torch.autograd.Function):
    @staticmethod
    def forward(fctx, layer, q, bmin, bmax, Qx, Ax, select=None):
        bt = layer.batch
        if (Qx is None) != (Ax is None):
            raise ValueError("Qx and Ax: give both or neither (update_Q_A takes both)")
        if Qx is not None and select is not None:
            raise ValueError("select: update_Q_A rebuilds every member, so Qx / Ax cannot be combined with a subset")
        if Qx is not None:
            a, b = bt._dev_args((Qx.detach(), (bt.B, bt.nnzQ), "Qx", "float64"), (Ax.detach(), (bt.B, bt.nnzA), "Ax", "float64"))
            bt.update_Q_A_device(a.value, b.value)
        det = lambda t: None if t is None else t.detach()
        if select is None:
            rc, out = bt.step_device(det(bmin), det(bmax), det(q), warm=layer.warm)
        else:
            # the step writes the selected rows only: x, y and the statuses of every member are read afterwards
            rc, out = bt.step_device(det(bmin), det(bmax), det(q), warm=layer.warm, out=bt._zeros("step", ("rejected",)), select=select)
            out["x"], out["y"] = bt.solution_device()
            out["status_val"], _ = bt.status_device()
        if rc != 0:
            raise ValueError("QPLayer: some member's bounds were refused (bmin > bmax): %r" % out["rejected"].nonzero().flatten().tolist())
        if layer.polish:
            # accepted members: the exact solution at their active set, returned and stored -- backward and jvp differentiate at the stored solution
            keys = ("res", "flag", "resid", "passes") + (("active",) if layer.replay else ())   # (the set the polish used: the recorded point's active set)
            pol_out = dict(x=out["x"], y=out["y"], **bt._zeros("polish", keys))
            pol = bt.polish_device(store=True, select=select, out=pol_out)
            layer.last_polish = {k: pol[k] for k in ("flag", "res", "resid", "passes")}
        fctx.layer, fctx.epoch, fctx.select = layer, bt.epoch, select
        fctx.replay = layer.replay
        if layer.replay:   # the point of THIS solve, for a backward() that may come any number of steps later
            if layer.polish:
                active = pol["active"]
            else:
                active = bt.active_device(out=bt._empty((bt.B, bt.m), "int64").zero_(), select=select)
            fctx.save_for_backward(out["x"], out["y"])
            fctx.active, fctx.status_val, fctx.matrix_epoch = active, out["status_val"].clone(), bt.matrix_epoch
        fctx.mark_non_differentiable(out["status_val"])
        return out["x"], out["y"], out["status_val"]

    @staticmethod
    def backward(fctx, gx, gy, _gs):
        """the adjoint of the state the batch holds, or with replay=True at the recorded point of this forward pass: the batch may then have been stepped
        any number of times since"""
        layer = fctx.layer
        bt = layer.batch
        if fctx.replay:
            if bt.matrix_epoch != fctx.matrix_epoch:
                raise RuntimeError("QPLayer.backward: the values of Q and A were updated after this forward pass; its recorded point is no longer valid")
            x, y = fctx.saved_tensors
            # the recorded statuses decide who is differentiated (the current ones are those of a later solve); the others keep zero rows
            select = ((fctx.status_val == SOLVED) | (fctx.status_val == DUAL_TERMINATED)).to(torch.int64)
            if fctx.select is not None:
                select = select * (fctx.select != 0).to(torch.int64)
            select, at = select.contiguous(), dict(at=(x.detach().contiguous(), y.detach().contiguous(), fctx.active))
        else:
            if bt.epoch != fctx.epoch:
                raise RuntimeError("QPLayer.backward: the batch was solved or updated again after this forward pass; its gradients are gone")
            select, at = getattr(fctx, "select", None), {}
        need = dict(zip(("dq", "dbmin", "dbmax", "dQx", "dAx"), fctx.needs_input_grad[1:6]))
        want = tuple(k for k, v in need.items() if v) + ("flag", "resid", "passes")
        gx = bt._empty((bt.B, bt.n)).zero_() if gx is None else gx.contiguous()
        if select is None:
            out = bt.adjoint_device(gx, None if gy is None else gy.contiguous(), want=want)
        else:   # rows of members that are not selected are not written: zero gradients
            out = bt.adjoint_device(gx, None if gy is None else gy.contiguous(), out=bt._zeros("adjoint", want), select=select, **at)
        layer.last_adjoint = {k: out[k] for k in ("flag", "resid", "passes")}
        return (None,) + tuple(out.get(k) for k in ("dq", "dbmin", "dbmax", "dQx", "dAx")) + (None,)

    @staticmethod
    def jvp(fctx, _layer, tq, tbmin, tbmax, tQx, tAx, _tselect=None):
        """forward-mode AD (torch.autograd.forward_ad): the tangent of the solved batch along the inputs' tangents (QpalmBatch.tangent_device)"""
        layer = fctx.layer
        bt = layer.batch
        if bt.epoch != fctx.epoch:
            raise RuntimeError("QPLayer.jvp: the batch was solved or updated again after this forward pass; its tangents are gone")
        con = lambda t: None if t is None else t.detach().contiguous()
        d = [con(t) for t in (tq, tbmin, tbmax, tQx, tAx)]
        if all(t is None for t in d):
            d[0] = bt._empty((bt.B, bt.n)).zero_()
        select = getattr(fctx, "select", None)
        if select is None:
            out = bt.tangent_device(*d, want=("dx", "dy", "flag", "resid", "passes"))
        else:   # rows of members that are not selected are not written: zero tangents
            out = bt.tangent_device(*d, out=bt._zeros("tangent", ("dx", "dy", "flag", "resid", "passes")), select=select)
        layer.last_tangent = {k: out[k] for k in ("flag", "resid", "passes")}
        return out["dx"], out["dy"], None


class QPLayer(torch.nn.Module):
    """x*(q, bmin, bmax[, Qx, Ax]) of a set-up QpalmBatch as a torch module.  warm: the warm start of every forward step, as step_device takes it
    (None = cold, "last" = every member's previous solution).  polish: polish every forward solve and store the result (see above).  sens_penalty: a
    number sets the batch's penalty floor for the adjoint, tangent and polish solves (QpalmBatch.sens_penalty); None leaves the
    batch's value alone.  replay: record every forward's point and differentiate there, so that backward() may come after later solves of the same batch
    (see above)."""

    def __init__(self, batch, warm=None, polish=False, sens_penalty=None, replay=False):
        super().__init__()
        if sens_penalty is not None:
            batch.sens_penalty = sens_penalty
        self.batch, self.warm, self.last_adjoint, self.last_tangent = batch, warm, None, None
        self.polish, self.last_polish = bool(polish), None
        self.replay = bool(replay)

    def forward(self, q=None, bmin=None, bmax=None, Qx=None, Ax=None, select=None):
        return _QPFunction.apply(self, q, bmin, bmax, Qx, Ax, select)
