"""What the step tests of Registration3DModel share (TEST infrastructure, imported as `from tests import step3d`): the
model builder of the per-term test files and the body of their "a replayed step equals the same step enqueued eagerly"
tests."""
import math

import torch

DEV = "cuda"


def step_model(shape, similarity, capture=False, **kw):
    """(model, A, B): Registration3DModel(shape, similarity=..., capture_step=capture, **kw) from seed 0, its flow head
    scaled up, and the two images of test_mind.mind_inputs on the device."""
    from dfmir_amd.registration3d import Registration3DModel
    from tests.test_mind import mind_inputs
    torch.manual_seed(0)
    m = Registration3DModel(shape, None, capture_step=capture, device=DEV, similarity=similarity, **kw)
    with torch.no_grad():
        m.netR.flow.weight.mul_(3e4)              # a flow of voxels, not of 1e-5 voxels
    A, B = (t.to(DEV) for t in mind_inputs((1, 1) + shape, 640))
    return m, A, B


def assert_replay_matches_eager(m, data, keys, extra=()):
    """m: a capture_step=True model.  Three steps on `data` (two eager ones, then the capture), then twice: a replayed step
    against the same step enqueued eagerly from the same restored state (weights, Adam moments) -- the losses, whose keys
    are `keys`, finite and within 1e-5 relative; regA (1e-6), flow (1e-5), the gradient arena (5e-5) and every
    (attribute, tol) of `extra` within tol of the eager tensor's maximum.  These are the numbers every caller had.  Returns
    the loss dicts of the two eager steps."""
    from dfmir_amd import ops
    names = [("regA", 1e-6), ("flow", 1e-5)] + list(extra)
    for _ in range(3):                                    # two eager steps, then the capture
        m.set_input(data); m.optimize_parameters()
    assert m._graph['graph'] is not None
    o = m.optimizer_R
    refs = []
    for _ in range(2):
        snap = (o.flat_p.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o._steps)
        m.set_input(data); m.optimize_parameters()          # replay
        torch.cuda.synchronize()
        got = (m.get_current_losses(), [getattr(m, k).clone() for k, _ in names] + [o.flat_g.clone()])
        with torch.no_grad():
            o.flat_p.copy_(snap[0]); o.exp_avg.copy_(snap[1]); o.exp_avg_sq.copy_(snap[2])
        o._steps = snap[3]
        ops.bump_weights_epoch()
        m._graph['force_eager'] = True
        m.set_input(data); m.optimize_parameters()          # the same step, eager
        m._graph['force_eager'] = False
        torch.cuda.synchronize()
        ref = (m.get_current_losses(), [getattr(m, k) for k, _ in names] + [o.flat_g])
        assert sorted(ref[0]) == sorted(keys)
        for k in ref[0]:
            assert math.isfinite(got[0][k])
            assert abs(got[0][k] - ref[0][k]) <= 1e-5 * max(abs(ref[0][k]), 1e-8), (k, got[0][k], ref[0][k])
        for x, y, (what, tol) in zip(got[1], ref[1], names + [("grads", 5e-5)]):
            err = float((x - y).detach().abs().max())
            ymax = float(y.detach().abs().max())
            assert err <= tol * ymax + 1e-12, (what, err, ymax)
        refs.append(ref[0])
    return refs
