"""The side stream the 3D network runs on beside the 2D network (one per thread and device).

`note_step_start` (PNA.forward) marks where the caller's stream stood when the step began; `side_stream_for`
(Net3D.forward) hands out the side stream ordered after that mark and after the batch's own assembly, or None when
the call pattern is another one.  `invalidate_step` (every model backward) makes an older mark stale.  The why and the
ordering rules are with NET3D_STREAM below.
"""
import os
import threading

import torch

_tls = threading.local()


def _side(device):
    pool = getattr(_tls, 'pool', None)
    if pool is None:
        pool = _tls.pool = {}
    s = pool.get(device.index)
    if s is None:
        s = pool[device.index] = torch.cuda.Stream(device=device)
    return s


# thread the peer exchange's side-stream context belongs to (dist.enable_native_sync / disable_native_sync), or None
BOUND_THREAD = None


def side_stream(device):
    """this thread's side stream on `device` (created on first use): the stream the 3D network runs on beside the 2D network"""
    return _side(torch.device(device))


# ---- the 3D network next to the 2D network ---------------------------------------------------------------------------
# Net3D is ~85 small launches per step (140k edges x 20 features: 5-15 us kernels that occupy a fraction of the chip)
# and is independent of PNA until the loss.  When the caller runs `model(g2d)` and then `model3d(g3d)` - the reference's
# forward_pass, trainer/self_supervised_trainer.py:24-29 - Net3D's kernels go to a side stream that only waits for (a)
# everything the main stream held when PNA.forward was ENTERED (so the previous optimizer step is in, PNA's own kernels
# are not) and (b) the event the batch carries from its own assembly (graph.py: BatchedMolGraph.ready_event).  The main
# stream waits for the side stream before Net3D.forward returns, so every consumer of its output is ordered as before;
# autograd runs the backward of Net3D on the same side stream and joins it.  Any other call pattern (no step-start
# mark, a backward pass in between, a foreign graph object without the event) keeps Net3D on the caller's stream.
# I3D_NET3D_STREAM=0 switches it off.
NET3D_STREAM = os.environ.get('I3D_NET3D_STREAM', '1') != '0'


def note_step_start(device):
    """PNA.forward entry: remember the main stream's position."""
    if not NET3D_STREAM:
        return
    ev = getattr(_tls, 'step_event', None)
    if ev is None:
        ev = _tls.step_event = torch.cuda.Event()
    stream = torch.cuda.current_stream(device)
    ev.record(stream)
    _tls.step_valid = (device.index, stream.cuda_stream, _generation[0])


_generation = [0]      # bumped by every model backward pass (any thread): a mark taken before it is stale


def invalidate_step():
    """a backward pass ran: parameters may change before the next forward"""
    _generation[0] += 1


def side_stream_for(graph_event, device):
    """The side stream, already ordered after the step-start mark and the batch's own event - or None."""
    if not NET3D_STREAM or graph_event is None:
        return None
    if BOUND_THREAD is not None and BOUND_THREAD != threading.get_ident():
        # dist.enable_native_sync bound the peer exchange's second context to the side stream of ANOTHER thread: this thread's
        # side stream has no context (its collectives would share the default one with the 2D network's stream)
        raise RuntimeError('3dinfomax_amd: synchronised BatchNorm (peer exchange) was set up on another thread; run the '
                           'training loop on the thread that called dist.setup / enable_native_sync')
    main = torch.cuda.current_stream(device)
    if getattr(_tls, 'step_valid', None) != (device.index, main.cuda_stream, _generation[0]):
        return None
    _tls.step_valid = None                      # one consumer per mark
    side = _side(device)
    side.wait_event(_tls.step_event)
    side.wait_event(graph_event)
    return side
