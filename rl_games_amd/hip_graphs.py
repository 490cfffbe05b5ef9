"""HIP graphs, host side: the package's one capture site (GraphCapturer), steps replayed from static copies of their inputs
(StepGraphs: the agents' rollout steps, the players' play steps) and an agent's update graphs (UpdateGraphs).  Which
launches a graph holds, and when one is used at all, is its owner's business (agent.py, play_engine.py)."""
import gc
import weakref

import torch


class GraphCaptureError(RuntimeError):
    """A HIP graph capture failed; nothing ran on the device and host mirrors were rolled back."""


class GraphCapturer:
    """Captures into one graph pool, made on first use.  forms: the ChainFormSet of the chains the bodies launch;
    optimizer: the one whose host mirrors they advance (None: a rollout or play step, which advances none)."""

    def __init__(self, forms, optimizer=None):
        self.forms, self.optimizer, self._pool, self._live = forms, optimizer, None, weakref.WeakSet()

    def capture(self, body):
        """-> body() as a HIP graph.  Capturing executes nothing on the device; the host mirrors that the body advances
        (the optimiser's step count and weights version, the weight forms' stamps) are restored afterwards, also when
        the capture fails (GraphCaptureError)."""
        if not self._live:          # (also: every graph of the pool is gone, and the allocator retired it with the last)
            self._pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        opt = self.optimizer
        mirrors = (opt.step_count, opt.weights_version) if opt is not None else None
        # No automatic garbage collection while the stream is capturing: a cycle that owns device objects of an
        # earlier graph (torch.cuda.graph collects once on entry, but the body allocates hundreds of Python objects)
        # would be finalised in the middle of the capture, and releasing device resources there aborts the process.
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            with self.forms.captured(), torch.cuda.graph(g, pool=self._pool, capture_error_mode='thread_local'):
                body()
        except Exception as e:
            raise GraphCaptureError('HIP graph capture failed') from e
        finally:
            if gc_was_enabled:
                gc.enable()
            if opt is not None:
                opt.step_count, opt.weights_version = mirrors
        self._live.add(g)
        return g


def _static_like(x):
    if x is None:
        return None
    if torch.is_tensor(x):
        return torch.empty_like(x, memory_format=torch.contiguous_format)
    return [_static_like(t) for t in x]


class StepGraphs:
    """Steps whose inputs must sit at fixed addresses, replayed as graphs.  Per key: static copies of the inputs, made on
    first use; per (key, index): the graph and what the body returned while it was recorded (the steps of a rollout - the
    indices - share the statics of their key; a play step has no index).  len(): the graphs."""

    def __init__(self, capturer):
        self._capturer, self._statics, self._graphs = capturer, {}, {}

    def __len__(self):
        return len(self._graphs)

    def clear(self):
        self._graphs.clear()
        self._statics.clear()

    def step(self, key, body, inputs=None, index=None):
        """Copy `inputs` - a dict of tensors, lists of tensors (RNN states) and Nones - into the statics of `key`, in
        its order; on first use capture body(**statics) (a GraphCaptureError leaves the statics and no graph); replay;
        -> the recorded result.  No inputs: body() reads what already sits at fixed addresses."""
        inputs = inputs or {}
        st = self._statics.get(key)
        if st is None:
            st = self._statics[key] = {k: _static_like(x) for k, x in inputs.items()}
        for k, x in inputs.items():
            if torch.is_tensor(x):
                st[k].copy_(x)
            else:
                for dst, src in zip(st[k] or (), x or ()):
                    dst.copy_(src)
        entry = self._graphs.get((key, index))
        if entry is None:
            out = []
            g = self._capturer.capture(lambda: out.append(body(**st)))
            entry = self._graphs[(key, index)] = (g, out[0])
        entry[0].replay()
        return entry[1]


class UpdateGraphs:
    """An agent's update graphs: minibatch[i] (forward / loss / backward of minibatch i) with `optimizer` behind each, or
    `epoch` (a whole mini-epoch); signature: what they bake in; norm_state: the agent's _norm_ready behind a captured
    minibatch, which the optimiser graph is captured to find."""

    def __init__(self):
        self.signature = None
        self.clear()

    def clear(self):
        """Forget every update graph.  (The signature stays: the next ones are captured under it.)"""
        self.minibatch, self.optimizer, self.epoch, self.norm_state = {}, None, None, None

    def refresh(self, signature):
        if signature != self.signature:
            self.clear()
            self.signature = signature
