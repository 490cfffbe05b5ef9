"""A plain MLP + linear head(s) trained on the fused chain kernels, without autograd.

What autograd does between a loss kernel and the optimiser for the networks of the reference's builder
(rl_games/algos_torch/network_builder.py:224-311: `actor_mlp` / `critic_mlp` = Linear + activation pairs, then `value` /
`logits` Linear heads) - forward with the activations kept, dZ of every hidden layer with the bias-gradient column sums,
the weight gradients - as the launches of the continuous actor's hot path: the input normaliser + hidden layers + heads
as ONE forward launch, the dX / activation-backward / bias-sum chain as ONE backward launch (csrc/mlp_chain*.hip,
`ops.MlpChain`), every weight gradient as the MFMA launch of csrc/mlp_dw.hip (`ops.MlpDwPlan`).

WeightGrads is the one piece of host code between a backward launch and the optimiser, for the engines of this module and
for mlp_engine.ManualMLP alike: which (dZ, X, grad) products the MFMA launch takes, its plans per shape, the column
sums and the loss partials its finalise launch finishes, and the library / narrow-kernel products of what is left.
plain_trunk, head_span and rnn_cell_declined are the shape checks the engines and the agents share; trunk_views and
trunk_jobs are the one statement of a trunk's weight-gradient list behind a chain backward.  RnnStations is the one copy
of what lies between the gate-input product and the recurrent features - the LSTM / GRU cell's buffers, gate bias,
ping-pong states, the sequence kernels' argument tuples, gate-gradient column sums and weight-gradient jobs - for
RecurrentChainNet and mlp_engine.ManualMLP alike; each engine keeps its own trunk and head stations around it.

Users: the central value network (central_value.py, one value column) and the discrete-action agent (discrete_agent.py:
[value | logits] behind a shared trunk, or one chain per trunk with `separate: True` as in ppo_cartpole.yaml).  The
continuous actor's engine is mlp_engine.ManualMLP (loss inside the backward launch, a per-layer trunk mode, HIP graphs).
RecurrentChainNet is the recurrent engine of the discrete agent and the central value critic: the trunk + gate-input
product as one chain, then RnnStations, an optional layer norm and the heads.  RecurrentChainPair drives two of them
- the separate actor / critic trunks of a continuous policy, each with its own RNN - with one paired sequence launch.  The
agents' rollout graphs read these chains too; they hold no pack launch, so the agent brings each chain's weight fragments
/ planes up to date in front of a replay along with its other chains (weight_forms.ChainFormSet.before_replay).
"""
import torch
from torch import nn

from . import ops

_DW_MAX_ITEMS = 8          # weight matrices / column-sum jobs of one ops.MlpDwPlan launch (csrc/mlp_dw.hip, kDwMaxLayers)
_ACT_NAMES = {nn.ELU: 'elu', nn.ReLU: 'relu', nn.Tanh: 'tanh', nn.Identity: 'None'}


def arena_layout(params, head_groups, first_vectors=()):
    """Physical arena order for `FlatArena(layout=...)`: every weight matrix first (parameters() order), then each
    group of head weights (adjacent, in the given order - one GEMM operand per group), then the vectors, then each
    group's biases.  Matrix sizes of the supported shapes are multiples of 4 floats, so the matrices stay 16-byte
    aligned; the logical (optimiser-state) order is untouched.  head_groups: lists of nn.Linear.
    first_vectors: vectors to put in front of the others - the trunk's biases directly behind the last matrix
    (RecurrentChainNet, mlp_engine.ManualMLP.layout): the pipelined forward kernels read up to 48 bytes past a matrix
    whose width is no multiple of 16 and accept that only when the bytes belong to another array of the SAME network
    (csrc/mlp_chain.hip, chain_pipe_fill) - sigma and the like come after them."""
    head_w = [m.weight for g in head_groups for m in g]
    head_b = [m.bias for g in head_groups for m in g]
    skip = {id(p) for p in head_w + head_b}
    rest = [p for p in params if id(p) not in skip]
    first = {id(p) for p in first_vectors}
    vecs = sorted((p for p in rest if p.dim() < 2), key=lambda p: id(p) not in first)      # (stable)
    return [p for p in rest if p.dim() >= 2] + head_w + vecs + head_b


def plain_trunk(trunk, identity_ok=True):
    """(linears, activation name) of an nn.Sequential of Linear + activation pairs with one activation kind - what an
    `ops.MlpChain` takes.  identity_ok=False: in front of an RNN, where a linear trunk is not a supported shape."""
    linears = [m for m in trunk if isinstance(m, nn.Linear)]
    acts = [m for m in trunk if not isinstance(m, nn.Linear)]
    if not linears or len(acts) != len(linears):
        raise NotImplementedError('unexpected MLP structure')
    name = _ACT_NAMES.get(type(acts[0]))
    if name is None or (name == 'None' and not identity_ok) or any(type(a) is not type(acts[0]) for a in acts):
        raise NotImplementedError('elu / relu / tanh / identity trunks only' if identity_ok else
                                  'elu / relu / tanh trunks only')
    if isinstance(acts[0], nn.ELU) and acts[0].alpha != 1.0:
        raise NotImplementedError('elu alpha != 1')
    if any(l.out_features % 4 for l in linears):
        raise NotImplementedError('hidden widths must be multiples of 4')
    return linears, name


def head_span(heads, arena):
    """(w [columns, K], w_grad, b [columns], b_grad, columns) of nn.Linear heads over the same K features whose weights
    (and biases) are adjacent in `arena`, in that order: their columns side by side, one GEMM operand."""
    columns = sum(h.out_features for h in heads)
    if len(heads) == 1:
        h = heads[0]
        return h.weight, h.weight.grad, h.bias, h.bias.grad, columns
    K = heads[0].in_features
    wp, wg = arena.span_of([h.weight for h in heads])
    bp, bg = arena.span_of([h.bias for h in heads])
    return wp.view(columns, K), wg.view(columns, K), bp, bg, columns


RNN_CELLS = 'a single-layer LSTM or GRU with 16/32/64/128 units'


def rnn_cell_declined(name, layers, units):
    """Why the sequence-persistent kernels do not take a recurrent cell ('lstm' / 'gru', layers, units), or None."""
    supported = {'lstm': ops.lstm_supported, 'gru': ops.gru_supported}.get(name)
    if supported is None or layers != 1 or not supported(units):
        return RNN_CELLS + ' only'
    return None


class WeightGrads:
    """The weight gradients of one backward pass, from the (dZ, X, grad) products the engine lists to finished
    gradients in the arena.  Everything inside the envelope of the MFMA launch (csrc/mlp_dw.hip: input columns a
    multiple of 4, contiguous 16-byte aligned operands, at most _DW_MAX_ITEMS matrices) is ONE `ops.MlpDwPlan` launch,
    the heaviest matrix's blocks first; its finalise launch also finishes up to _DW_MAX_ITEMS bias column sums and the
    PPO loss partials.  What is left - a first layer over 9 state features, say - is a library product each, or with
    `narrow` the narrow kernel of csrc/mlp_narrow.hip where it applies (the two give different bits).
    mfma=False: no MFMA launch at all.  Plans (and the shapes the launch declined) are kept per shape key.
    form: the product form of the MFMA launch (ops.MlpDwPlan.launch) - None: the library's choice, 'exact': f32 products
    whatever maxima the step carries (an agent on `chain_products: exact`)."""

    def __init__(self, mfma=True, narrow=False):
        self.mfma, self.narrow = bool(mfma), bool(narrow)
        self.form = None
        self._plans = {}
        self.last_dw_path = None            # 'mfma' / 'library': whether the last finish() had an MFMA launch
        self.last_dw_jobs = None            # (jobs, plan, maxima) of the last MFMA launch: bench.py times it after the run
        self.last_dw_library_jobs = None    # torch.mm products of the last finish()

    def _plan(self, fast, rows):
        shapes = [tuple(j[2].shape) for j in fast]
        key = (rows,) + tuple(shapes)
        plan = self._plans.get(key)
        if plan is None:
            try:
                plan = ops.MlpDwPlan(shapes, rows, fast[0][2].device)
            except NotImplementedError:
                plan = False
            self._plans[key] = plan
        return plan

    def finish(self, jobs, rows, colsums=(), loss_finalize=None, norm=None, maxima=None):
        """jobs: (dZ [rows, No], X [rows, Mi], grad [No, Mi][, layer index]); colsums: (partials, blocks, cols, gradient
        vector).  loss_finalize: ops.loss_finalize_desc(...) - folded into the finalise launch when there is one,
        launched on its own otherwise.  norm = (partials, grad_scale, step_counter): see ops.MlpDwPlan.launch; returns
        the number of valid norm partials, or None when the gradient norm was not produced (a gradient of this step did
        not come out of that launch, or the partials are too few for its finalise grid: the caller's grad_sumsq launch
        takes over instead of an error in the middle of an epoch).  maxima = (ops.MlpChain.gradient_maxima() of the
        step, rows per entry) or None: the launch runs its fp16 form when every job in it carries the layer index that
        names dZ's row of the maxima, else its bf16 form."""
        fast = [j for j in jobs if self.mfma and j[2].shape[1] % 4 == 0 and j[2].shape[1] >= 4
                and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in j[:3])]
        fast.sort(key=lambda j: -j[2].numel())
        plan = self._plan(fast, rows) if 0 < len(fast) <= _DW_MAX_ITEMS else None
        if not plan:
            fast = []
        slow = [j for j in jobs if not any(j is f for f in fast)]
        colsums = list(colsums)
        norm_blocks = None
        if plan:
            launched, colsums = colsums[:_DW_MAX_ITEMS], colsums[_DW_MAX_ITEMS:]
            # the gradient norm as well when every gradient of the step is written by this launch
            whole = (norm is not None and not slow and not colsums and loss_finalize is not None
                     and norm[0].numel() >= plan.finalize_blocks(launched, loss_finalize))
            mx = None
            if maxima is not None and self.form != 'exact' and all(len(j) == 4 for j in fast):
                # X is split under the forward's fixed scales: normalised observations (layer 0) / hidden activations
                mx = (maxima[0], [j[3] for j in fast],
                      [ops.SPLIT_SCALE_OBS_NORM if j[3] == 0 else ops.SPLIT_SCALE_HIDDEN for j in fast], maxima[1])
            triples = [j[:3] for j in fast]
            form = {} if self.form is None else {'form': self.form}        # (None: the launch as it always was)
            blocks = plan.launch(triples, launched, loss_finalize, norm if whole else None, maxima=mx, **form)
            norm_blocks = blocks if whole else None
            loss_finalize = None
            self.last_dw_jobs = (triples, plan, mx)
        if loss_finalize is not None:
            ops.ppo_loss_finalize_from(loss_finalize, jobs[0][2].device)
        for part, nb, cols, out in colsums:
            ops.colsum_finalize(part, nb, cols, out)
        self.last_dw_path = 'mfma' if plan else 'library'
        self.last_dw_library_jobs = 0
        for dz, x, g in (j[:3] for j in slow):
            if (self.narrow and g.shape[1] <= ops.NARROW_MAX and g.shape[0] <= 256 and dz.stride(1) == 1
                    and x.stride(1) == 1 and g.is_contiguous()):
                ops.narrow_dw(dz, x, g)            # a first layer over a few observations (obs 3)
            else:
                torch.mm(dz.t(), x, out=g)
                self.last_dw_library_jobs += 1
        return norm_blocks


def trunk_views(linears, acts, dzs, partials, rows, nblk):
    """The first `rows` rows of a trunk's activation and dZ buffers, and the `nblk` partial rows per layer a chain
    backward over them writes (ops.MlpChain.num_blocks) - what ops.MlpChain.backward and trunk_jobs take."""
    return ([h[:rows] for h in acts], [d[:rows] for d in dzs],
            [p[:nblk * l.out_features] for p, l in zip(partials, linears)])


def trunk_jobs(linears, x, acts, dzs, parts, nblk):
    """(jobs, colsums) of a trunk for WeightGrads.finish behind a chain backward, last layer first: (dZ, X, W.grad,
    layer) with X the layer below's activations - `x` under layer 0 - and (partials, blocks, cols, b.grad).  The layer
    index names dZ's row of the backward's gradient maxima; finish() reads it only when it is given those."""
    jobs, colsums = [], []
    for l in range(len(linears) - 1, -1, -1):
        lin = linears[l]
        jobs.append((dzs[l], acts[l - 1] if l > 0 else x, lin.weight.grad, l))
        colsums.append((parts[l], nblk, lin.out_features, lin.bias.grad))
    return jobs, colsums


class RnnStations:
    """The stations of a single-layer LSTM / GRU between the gate-input product and the features the heads read, for
    every engine that has one (RecurrentChainNet, mlp_engine.ManualMLP): the cell's buffers, the bias of the gate-input
    product, the ping-pong final states, the argument tuples of the sequence-persistent kernels (csrc/lstm*.hip,
    csrc/gru*.hip) and, behind their backward, the bias column sums and the two weight-gradient jobs.  No trunk, no
    layer norm, no heads and no loss: the engine writes `gates[:rows]`, reads `rnn_out[:rows]`, and hands
    `d_rnn_out[:rows]` (or a buffer of its own) to backward_args.
    rnn: the torch.nn.LSTM / GRU module (parameters only); rows: the most rows of a forward."""

    def __init__(self, rnn, rows, device):
        self.lstm = rnn if isinstance(rnn, nn.LSTM) else None
        self.gru = rnn if isinstance(rnn, nn.GRU) else None
        if self.lstm is None and self.gru is None:
            raise NotImplementedError('LSTM or GRU only')
        H = rnn.hidden_size
        if (rnn_cell_declined('lstm' if self.lstm is not None else 'gru', rnn.num_layers, H) or rnn.bidirectional
                or not rnn.bias or getattr(rnn, 'proj_size', 0)):
            raise NotImplementedError(RNN_CELLS + ' only')
        self.rnn, self.Hr = rnn, H
        self.Gr = G = (4 if self.lstm is not None else 3) * H        # gate columns
        # the bias of the gate-input product.  LSTM: b_ih + b_hh, summed into bias_sum by every forward.  GRU: b_hn is
        # multiplied by r inside the cell, so only b_ih belongs to the input side - bias_ih_l0 itself; the kernel adds
        # b_hh.
        if self.lstm is not None:
            self.gate_bias = self.bias_sum = torch.empty(G, device=device)
        else:
            self.gate_bias, self.bias_sum = rnn.bias_ih_l0, None

        def buf(cols):
            return torch.empty(rows, cols, device=device)
        self.gates, self.rnn_out, self.d_rnn_out, self.hprev = buf(G), buf(H), buf(H), buf(H)
        self.gate_partials = torch.empty(ops.act_bwd_blocks(rows, G) * G, dtype=torch.float64, device=device)
        if self.lstm is not None:
            self.d_gates, self.c_all = buf(G), buf(H)
        else:
            self.hn_all = buf(H)                            # W_hn h + b_hn, before the gating by r
            self.d_gx, self.d_gh = buf(G), buf(G)           # gradient of the input side / of the hidden side
            self.gate_partials_h = torch.empty_like(self.gate_partials)
        # final states of the last keep=False forward (LSTM: h and c, GRU: h), ping-pong so that a caller may feed them
        # back in
        nstates = 2 if self.lstm is not None else 1
        self._state_buf = [[torch.empty(1, rows, H, device=device) for _ in range(nstates)] for _ in range(2)]
        self.last_states = None
        self._kept = None

    @torch.no_grad()
    def forward_args(self, rows, rnn_states, dones, seq_length, keep):
        """Checks the shapes, sums the LSTM's biases (a launch) and returns the arguments of ops.lstm_seq_forward /
        gru_seq_forward, without seq_len, for `rows` rows ordered (sequence, t) with `seq_length` steps each.
        rnn_states = (h0, c0) - GRU: (h0,) - contiguous [1, rows / seq_length, H]; dones [rows] resets the state
        entering a step (or None).  keep=True has the kernel keep what backward_args reads and leaves the state buffers
        alone (they hold the live rollout state); keep=False (a rollout step, get_values) keeps nothing and puts the
        final states into whichever buffer pair the inputs do not live in - `last_states`, None after keep=True."""
        S = rows // seq_length
        if S * seq_length != rows:
            raise ValueError(f'rows ({rows}) must be a multiple of seq_length ({seq_length})')
        if dones is not None:
            dones = dones.reshape(-1)
            if dones.dtype != torch.uint8 or not dones.is_contiguous():
                dones = dones.to(torch.uint8).contiguous()
        rnn, H = self.rnn, self.Hr
        h0 = rnn_states[0][0]
        c0 = rnn_states[1][0] if self.lstm is not None else None
        if h0.shape != (S, H) or not h0.is_contiguous() or not (c0 is None or (c0.shape == (S, H) and c0.is_contiguous())):
            raise ValueError(f'rnn_states must be contiguous [1, {S}, {H}] tensors')
        if self.lstm is not None:
            torch.add(rnn.bias_ih_l0, rnn.bias_hh_l0, out=self.bias_sum)
        if keep:
            self._kept = (rows, c0, dones, seq_length)
            self.last_states = None
            kept = ((self.c_all if self.lstm is not None else self.hn_all)[:rows], self.hprev[:rows])
            finals = (None,) * len(self._state_buf[0])
        else:
            pair = self._state_buf[1 if h0.data_ptr() == self._state_buf[0][0].data_ptr() else 0]
            self.last_states = tuple(t[:, :S] for t in pair)
            kept = (None, None)
            finals = tuple(t[0] for t in self.last_states)
        gates, out = self.gates[:rows], self.rnn_out[:rows]
        if self.lstm is not None:
            return (gates, rnn.weight_hh_l0, h0, c0, dones, out) + kept + finals
        return (gates, rnn.weight_hh_l0, rnn.bias_hh_l0, h0, dones, out) + kept + finals

    def sequence(self, direction, args, seq_length):
        """The sequence kernel as a launch of its own: direction 'forward' / 'backward', args from forward_args /
        backward_args."""
        ops.rnn_seq('lstm' if self.lstm is not None else 'gru', direction, [args], seq_length)

    @property
    def seq_length(self):
        """Steps per sequence of the last keep=True forward: the backward kernel's seq_len."""
        return self._kept[3]

    def backward_args(self, d_out):
        """The arguments of ops.lstm_seq_backward / gru_seq_backward, without seq_len, from d_out [rows, H] and what
        the last keep=True forward kept."""
        rows, c0, dones, _ = self._kept
        gates, w_hh = self.gates[:rows], self.rnn.weight_hh_l0
        if self.lstm is not None:
            return (gates, self.c_all[:rows], c0, dones, w_hh, d_out, self.d_gates[:rows])
        return (gates, self.hn_all[:rows], self.hprev[:rows], dones, w_hh, d_out, self.d_gx[:rows], self.d_gh[:rows])

    def gate_gradients(self, rnn_in):
        """Behind the backward sequence kernel: the column sums of the gate gradients (one launch, GRU two).  Returns
        (dg, jobs, colsums): dg, the gradient of the gate-input product that the trunk's backward starts from; the two
        weight-gradient jobs, W_hh's and - over rnn_in [rows, input], the trunk's features - W_ih's; the two bias
        gradients' column-sum jobs."""
        rows, G, rnn = self._kept[0], self.Gr, self.rnn
        nbg = ops.act_bwd_blocks(rows, G)
        gpart = gpart_h = self.gate_partials[:nbg * G]
        if self.lstm is not None:
            dg = dgh = self.d_gates[:rows]
            ops.act_bwd_colsum(dg, None, dg, 0, gpart, nbg)                  # identity: column sums only
        else:
            # dg = d_gx: the input side - W_ih, b_ih and the trunk; dgh = d_gh: the hidden side - W_hh, b_hh
            dg, dgh = self.d_gx[:rows], self.d_gh[:rows]
            gpart_h = self.gate_partials_h[:nbg * G]
            ops.act_bwd_colsum(dg, None, dg, 0, gpart, nbg)
            ops.act_bwd_colsum(dgh, None, dgh, 0, gpart_h, nbg)
        jobs = [(dgh, self.hprev[:rows], rnn.weight_hh_l0.grad), (dg, rnn_in, rnn.weight_ih_l0.grad)]
        colsums = [(gpart, nbg, G, rnn.bias_ih_l0.grad), (gpart_h, nbg, G, rnn.bias_hh_l0.grad)]   # LSTM: d b_hh = d b_ih
        return dg, jobs, colsums


class ChainNet:
    """trunk: nn.Sequential of Linear + activation pairs; heads: list of nn.Linear over the trunk's output whose
    weights (and biases) are adjacent in `arena`, in that order (arena_layout) - their columns side by side are the
    chain's last layer.  Raises NotImplementedError for networks outside the kernels' envelope."""

    def __init__(self, trunk, heads, arena, max_rows, infer_rows=0):
        self.linears, name = plain_trunk(trunk)
        heads = list(heads)
        if any(h.in_features != self.linears[-1].out_features for h in heads):
            raise NotImplementedError('heads must read the last hidden layer')
        self.head_w, self.head_w_grad, self.head_b, self.head_b_grad, self.head_cols = head_span(heads, arena)
        dev = self.head_w.device
        widths = [l.out_features for l in self.linears]
        layers = [(l.weight, l.bias, name) for l in self.linears] + [(self.head_w, self.head_b, 'None')]
        self.chain = ops.MlpChain(layers, dev, weights_version=arena.weights_token)
        self.Hs = [torch.empty(max_rows, w, device=dev) for w in widths]
        self.dA = [torch.empty(max_rows, w, device=dev) for w in widths]
        self.heads = torch.empty(max_rows, self.head_cols, device=dev)
        self.d_heads = torch.empty(max_rows, self.head_cols, device=dev)
        self.xn = torch.empty(max_rows, self.linears[0].in_features, device=dev)
        self.infer_heads = torch.empty(infer_rows, self.head_cols, device=dev)
        nb = (max_rows + 15) // 16                          # one partial row per 16-row group at most
        self.partials = [torch.empty(nb * w, dtype=torch.float64, device=dev) for w in widths]
        self.weight_grads = WeightGrads()
        self._rows = 0
        self._x = None

    @property
    def last_dw_path(self):
        return self.weight_grads.last_dw_path

    @torch.no_grad()
    def forward(self, x, rms, eps):
        """x [rows, in] RAW inputs; rms = (running_mean, running_var) or None.  Returns the heads [rows, head_cols]
        and keeps what backward() reads."""
        rows = x.shape[0]
        if not x.is_contiguous():
            x = x.contiguous()
        heads = self.heads[:rows]
        xn = self.xn[:rows] if rms is not None else None
        self.chain.forward(x, heads, act_out=[h[:rows] for h in self.Hs], rms=rms, eps=eps, xn_out=xn)
        self._rows, self._x = rows, (xn if rms is not None else x)
        return heads

    @torch.no_grad()
    def infer(self, x, rms, eps):
        """Inference forward of a rollout step: x [rows, in] RAW inputs with any row stride (e.g. the buffer slot of the
        step), normalised inside the launch with the statistics as they are (eval mode).  Keeps no activations; the heads
        go to a buffer of their own (`infer_rows` rows, grown when `rows` is larger).  Returns heads [rows, head_cols]."""
        rows = x.shape[0]
        self.reserve_infer(rows)
        heads = self.infer_heads[:rows]
        self.chain.forward(x, heads, rms=rms, eps=eps)
        return heads

    def reserve_infer(self, rows):
        """Allocate infer()'s heads buffer for `rows` rows now (not on first use, e.g. inside a graph capture)."""
        if self.infer_heads.shape[0] < rows:
            self.infer_heads = torch.empty(rows, self.head_cols, device=self.infer_heads.device)

    @torch.no_grad()
    def backward(self):
        """d loss / d heads in self.d_heads[:rows] -> every gradient of the network in the arena."""
        rows = self._rows
        d_heads = self.d_heads[:rows]
        nblk = self.chain.num_blocks(rows, 1)
        acts, dzs, parts = trunk_views(self.linears, self.Hs, self.dA, self.partials, rows, nblk)
        self.chain.backward(d_heads, acts, dzs, parts)
        jobs, colsums = trunk_jobs(self.linears, self._x, acts, dzs, parts, nblk)
        if self.head_cols == 1:
            # one output column - a weighted column sum of the last activations, and the sum of d heads
            torch.mv(acts[-1].t(), d_heads.view(-1), out=self.head_w_grad.view(-1))
        else:
            jobs.insert(0, (d_heads, acts[-1], self.head_w_grad))
        torch.sum(d_heads, dim=0, out=self.head_b_grad)
        self.weight_grads.finish(jobs, rows, colsums)


class RecurrentChainNet:
    """One trunk of a recurrent policy without autograd:
        obs -> [Linear + act] x L -> W_ih x + b -> LSTM | GRU (one layer, 16 / 32 / 64 / 128 units)
            -> optional nn.LayerNorm(units) -> heads
    for arbitrary head columns (`heads`: nn.Linear modules over the recurrent features, adjacent in `arena` as for
    ChainNet).  The normaliser, the trunk and the gate-input product are one `ops.MlpChain` launch whose last (linear)
    layer is W_ih; the sequence-persistent kernels of csrc/lstm*.hip / csrc/gru*.hip (`stations`: the RnnStations that
    mlp_engine.ManualMLP's recurrent branch runs on too), the layer norm of csrc/rnn_layer_norm.hip and the head product
    follow.  backward() runs the same stations in reverse from `d_heads` and finishes every weight gradient in one
    `ops.MlpDwPlan` launch.
    trunk: nn.Sequential of Linear + activation pairs; rnn: the torch.nn.LSTM / GRU module (parameters only);
    layer_norm: nn.LayerNorm or None.  max_rows: rows of a training minibatch, infer_rows: rows of a rollout step.
    value_tail (a central value critic: `heads` is one value column): the head, the clipped value loss and the head's
    backward are one launch of csrc/rnn_value_tail.hip - forward(keep=True, value_loss=...) runs it in place of
    heads -> loss kernel -> head dX -> bias sum -> 1 x H weight-gradient job and leaves the loss partials in
    `loss_partials[:loss_blocks]`; backward() then starts at the recurrent features.
    Raises NotImplementedError for networks outside the kernels' envelope - there is no per-layer fallback."""

    def __init__(self, trunk, rnn, layer_norm, heads, arena, max_rows, infer_rows=0, value_tail=False):
        self.linears, name = plain_trunk(trunk, identity_ok=False)
        rows = max(int(max_rows), int(infer_rows), 1)
        self.stations = st = RnnStations(rnn, rows, self.linears[0].weight.device)
        self.lstm, self.gru, self.rnn, self.Hr, self.Gr = st.lstm, st.gru, st.rnn, st.Hr, st.Gr
        H = st.Hr
        if rnn.input_size != self.linears[-1].out_features:
            raise NotImplementedError(RNN_CELLS + ' behind the trunk only')
        if layer_norm is not None and (tuple(layer_norm.normalized_shape) != (H,) or layer_norm.weight is None
                                       or layer_norm.bias is None):
            raise NotImplementedError('layer norm over the recurrent features with weight and bias only')
        self.ln = layer_norm
        heads = list(heads)
        if any(h.in_features != H for h in heads):
            raise NotImplementedError('heads must read the recurrent features')
        self.head_w, self.head_w_grad, self.head_b, self.head_b_grad, self.head_cols = head_span(heads, arena)
        C = self.head_cols
        dev = self.head_w.device
        layers = [(l.weight, l.bias, name) for l in self.linears] + [(rnn.weight_ih_l0, st.gate_bias, 'None')]
        self.chain = ops.MlpChain(layers, dev, weights_version=arena.weights_token)
        self._head_mfma = (C <= 64 and ops.mlp_rowgemm_supported(H, H) and self.head_w.data_ptr() % 16 == 0)
        self.value_tail = bool(value_tail)
        if self.value_tail and (len(heads) != 1 or C != 1):
            raise NotImplementedError('the value tail takes one value column')
        widths = [l.out_features for l in self.linears]

        def buf(cols, dtype=torch.float32):
            return torch.empty(rows, cols, dtype=dtype, device=dev)
        self.Hs = [buf(w) for w in widths]
        self.dA = [buf(w) for w in widths]
        self.xn = buf(self.linears[0].in_features)
        self.heads, self.d_heads = buf(C), buf(C)
        nb = (rows + 15) // 16                              # one partial row per 16-row group at most
        self.partials = [torch.empty(nb * w, dtype=torch.float64, device=dev) for w in widths]
        if self.ln is not None:
            self.ln_out, self.d_ln_out, self.ln_stats = buf(H), buf(H), buf(2)
            nbl = max(ops.rnn_layer_norm_blocks(rows, H), 1)
            self.ln_partials = [torch.empty(nbl * H, dtype=torch.float64, device=dev) for _ in range(2)]
        if self.value_tail:
            nbt = max(ops.rnn_value_tail_blocks(rows, H), 1)
            self.loss_partials = torch.empty(nbt * 7, dtype=torch.float64, device=dev)
            self.tail_partials = [torch.empty(nbt * H, dtype=torch.float64, device=dev),
                                  torch.empty(nbt, dtype=torch.float64, device=dev)]
            self.loss_blocks = 0
        self.weight_grads = WeightGrads()
        self._rows = self._fwd_rows = 0
        self._x = None

    @property
    def last_dw_path(self):
        return self.weight_grads.last_dw_path

    @property
    def last_states(self):
        return self.stations.last_states

    @torch.no_grad()
    def forward(self, x_raw, rms, eps, rnn_states, dones, seq_length, keep, value_loss=None):
        """x_raw [rows, in] RAW inputs, rows ordered (sequence, t) with `seq_length` steps each; rms = (running_mean,
        running_var) or None - the launch normalises on the way in.  rnn_states = (h0, c0) - GRU: (h0,) - of shape
        [1, rows / seq_length, H]; dones [rows] u8 resets the state entering a step (or None).  Returns the heads
        [rows, head_cols].  keep=True retains what backward() reads and leaves the state buffers alone (they hold the
        live rollout state); keep=False (a rollout step, get_values) keeps nothing and leaves the final states in
        `last_states`, in whichever buffer pair the inputs do not live in.
        value_tail engines: value_loss = (old_values [rows], returns [rows], mask [rows] or None, sum(mask) [1] or None,
        e_clip, clip_value) with keep=True - the launch also writes d_heads and the gradient of the recurrent features,
        and the loss partials for ops.ppo_loss_finalize; keep=False ends in the value column alone."""
        if self.value_tail and keep and value_loss is None:
            raise ValueError('a value-tail engine needs value_loss=(old_values, returns, mask, mask_sum, e_clip, clip_value) '
                             'for a training forward')
        if value_loss is not None and not (self.value_tail and keep):
            raise ValueError('value_loss goes with keep=True on a value-tail engine')
        args = self.forward_pre_rnn(x_raw, rms, eps, rnn_states, dones, seq_length, keep)
        self.stations.sequence('forward', args, seq_length)
        return self.forward_post_rnn(keep, value_loss)

    # forward() and backward() in three stations each - in front of the sequence kernel, the kernel, behind it - so that
    # RecurrentChainPair can run two engines' sequence kernels as one paired launch.  forward() / backward() launch
    # what they always launched, in the same order.
    @torch.no_grad()
    def forward_pre_rnn(self, x_raw, rms, eps, rnn_states, dones, seq_length, keep):
        """Trunk + gate-input product.  Returns the arguments of ops.lstm_seq_forward / gru_seq_forward (without
        seq_len) for the sequence kernel that has to run next."""
        rows = x_raw.shape[0]
        if not x_raw.is_contiguous() and (keep or x_raw.stride(-1) != 1):
            x_raw = x_raw.contiguous()
        args = self.stations.forward_args(rows, rnn_states, dones, seq_length, keep)
        gates = args[0]
        if keep:
            xn = self.xn[:rows] if rms is not None else None
            self.chain.forward(x_raw, gates, act_out=[h[:rows] for h in self.Hs], rms=rms, eps=eps, xn_out=xn)
            self._x = xn if rms is not None else x_raw       # what the first layer's weight gradient reads
        else:
            self.chain.forward(x_raw, gates, rms=rms, eps=eps)
        self._fwd_rows = rows
        return args

    @torch.no_grad()
    def forward_post_rnn(self, keep, value_loss=None, heads_out=None):
        """Layer norm and head product of the rows forward_pre_rnn saw.  heads_out: a [rows, head_cols] view (unit
        column stride) to write the heads into in place of the engine's own buffer (plain head mode)."""
        rows, H, st = self._fwd_rows, self.Hr, self.stations
        out = feat = st.rnn_out[:rows]
        if self.ln is not None:
            feat = self.ln_out[:rows]
            ops.rnn_layer_norm_forward(out, self.ln.weight, self.ln.bias, self.ln.eps, feat,
                                       self.ln_stats[:rows] if keep else None)
        heads = self.heads[:rows] if heads_out is None else heads_out
        if self.value_tail and keep:
            old_values, returns, mask, mask_sum, e_clip, clip_value = value_loss
            self.loss_blocks = nbt = ops.rnn_value_tail_blocks(rows, H)
            d_feat = (self.d_ln_out if self.ln is not None else st.d_rnn_out)[:rows]
            ops.rnn_value_tail(feat, self.head_w.view(-1), self.head_b, old_values, returns, heads.view(-1),
                               self.d_heads[:rows].view(-1), d_feat, self.loss_partials, self.tail_partials[0],
                               self.tail_partials[1], nbt, e_clip, clip_value, mask, mask_sum)
        elif self.value_tail:
            ops.rnn_value_head(feat, self.head_w.view(-1), self.head_b, heads.view(-1))
        elif self._head_mfma:
            ops.mlp_linear_act_forward(feat, self.head_w, self.head_b, heads, act_kind=0)
        else:
            torch.addmm(self.head_b, feat, self.head_w.t(), out=heads)
        if keep:
            self._rows = rows
        return heads

    @torch.no_grad()
    def backward(self):
        """d loss / d heads in self.d_heads[:rows] -> every gradient of the network in the arena (overwritten)."""
        args = self.backward_pre_rnn()
        self.stations.sequence('backward', args, self.stations.seq_length)
        self.backward_post_rnn()

    @torch.no_grad()
    def backward_pre_rnn(self):
        """Head dX and layer-norm backward.  Returns the arguments of ops.lstm_seq_backward / gru_seq_backward (without
        seq_len) for the sequence kernel that has to run next."""
        rows, H, st = self._rows, self.Hr, self.stations
        d_heads = self.d_heads[:rows]
        d_out = st.d_rnn_out[:rows]
        d_feat = self.d_ln_out[:rows] if self.ln is not None else d_out
        C = self.head_cols
        if self.value_tail:
            pass                                            # (the tail launch of the forward wrote d_feat)
        elif C <= ops.NARROW_MAX:
            ops.narrow_dx(d_heads, self.head_w, d_feat)
        elif ops.mlp_rowgemm_supported(C, C) and d_heads.data_ptr() % 16 == 0:
            ops.mlp_linear_act_backward(d_heads, self.head_w, None, d_feat, 0)
        else:
            torch.mm(d_heads, self.head_w, out=d_feat)
        colsums = []                                        # (partials, blocks, cols, gradient vector)
        if self.value_tail:
            nbt = self.loss_blocks
            colsums += [(self.tail_partials[0][:nbt * H], nbt, H, self.head_w_grad.view(-1)),
                        (self.tail_partials[1][:nbt], nbt, 1, self.head_b_grad)]
        if self.ln is not None:
            nbl = ops.rnn_layer_norm_blocks(rows, H)
            pg, pb = (p[:nbl * H] for p in self.ln_partials)
            ops.rnn_layer_norm_backward(d_feat, st.rnn_out[:rows], self.ln_stats[:rows], self.ln.weight, d_out, pg, pb,
                                        nbl)
            colsums += [(pg, nbl, H, self.ln.weight.grad), (pb, nbl, H, self.ln.bias.grad)]
        self._bwd_colsums = colsums
        return st.backward_args(d_out)

    @torch.no_grad()
    def backward_post_rnn(self):
        """From the gate gradients down: bias column sums, the trunk's dX chain, every weight gradient."""
        rows, st = self._rows, self.stations
        d_heads = self.d_heads[:rows]
        feat = (self.ln_out if self.ln is not None else st.rnn_out)[:rows]
        nblk = self.chain.num_blocks(rows, 1)
        acts, dzs, parts = trunk_views(self.linears, self.Hs, self.dA, self.partials, rows, nblk)
        dg, jobs, gate_colsums = st.gate_gradients(acts[-1])
        # dX chain of the trunk in one launch, from d gates down (the chain's "head" layer is W_ih)
        self.chain.backward(dg, acts, dzs, parts)
        if not self.value_tail:
            jobs.insert(0, (d_heads, feat, self.head_w_grad))
            torch.sum(d_heads, dim=0, out=self.head_b_grad)
        trunk, trunk_colsums = trunk_jobs(self.linears, self._x, acts, dzs, parts, nblk)
        # (bias / layer-norm gradients finished by the same finalise launch, as many as it takes)
        self.weight_grads.finish(jobs + trunk, rows, self._bwd_colsums + gate_colsums + trunk_colsums)


def paired_launch_pays(cell, hidden, direction, num_seqs, seq_len):
    """Is the paired sequence launch at least as fast as the two single launches (profiles/separate_rnn.txt, 1.)?  Every
    measured shape class but one: the 128-unit LSTM forward at T = 1 once the paired grid holds more workgroups than
    the chip has CUs (2 * ceil(S / 16) > 256) - 1.08 x the two launches at S = 4,096.  The outputs are the same bits
    either way."""
    return not (cell == 'lstm' and hidden == 128 and direction == 'forward' and seq_len == 1
                and 2 * ((num_seqs + 15) // 16) > 256)


class RecurrentChainPair:
    """Separate actor / critic trunks, each with its own RNN (`separate: True`, network_builder.py:272-277, :372-421):
    two RecurrentChainNet - the actor's over the `mu` head, the critic's over the `value` head, plain head mode - driven
    side by side so that their sequence kernels run as ONE paired launch (csrc/rnn_seq.hpp, "paired launches":
    bit-identical to the two single launches).  Everything else stays the launches of the two engines.
    paired=False, or two RNNs that differ in cell or width (the reference's builder makes them alike, but the
    constructor takes modules): two single launches.  So does the one shape class at which the paired launch measured
    slower (paired_launch_pays).
    The states travel in the model's order, the actor's in front of the critic's (get_default_rnn_state)."""

    def __init__(self, actor_trunk, actor_rnn, actor_ln, mu, critic_trunk, critic_rnn, critic_ln, value, arena, max_rows,
                 infer_rows=0, paired=True):
        self.actor = RecurrentChainNet(actor_trunk, actor_rnn, actor_ln, [mu], arena, max_rows, infer_rows=infer_rows)
        self.critic = RecurrentChainNet(critic_trunk, critic_rnn, critic_ln, [value], arena, max_rows,
                                        infer_rows=infer_rows)
        if self.critic.head_cols != 1:
            raise NotImplementedError('one value column only')
        self.lstm = self.actor.lstm is not None
        same = (type(actor_rnn) is type(critic_rnn) and self.actor.Hr == self.critic.Hr)
        self.paired = bool(paired) and same
        self._states_each = 2 if self.lstm else 1
        if (2 if self.critic.lstm is not None else 1) != self._states_each:
            raise NotImplementedError('two RNNs of one cell only')
        # a rollout step's heads side by side, [value | mu]: what ops.rollout_policy_head reads
        A = self.actor.head_cols
        self.joint_heads = torch.empty(max(int(infer_rows), 1), 1 + A, device=self.actor.heads.device)
        self.last_states = None
        self._T = 1

    @property
    def chains(self):
        return [self.actor.chain, self.critic.chain]

    @property
    def last_dw_path(self):
        return self.actor.last_dw_path

    def _sequence(self, direction, a_args, b_args, seq_length):
        cell = 'lstm' if self.lstm else 'gru'
        if self.paired and paired_launch_pays(cell, self.actor.Hr, direction, a_args[0].shape[0] // seq_length, seq_length):
            ops.rnn_seq(cell, direction, [a_args, b_args], seq_length)
        else:
            self.actor.stations.sequence(direction, a_args, seq_length)
            self.critic.stations.sequence(direction, b_args, seq_length)

    @torch.no_grad()
    def forward(self, x_raw, rms, eps, rnn_states, dones, seq_length, keep):
        """The arguments of RecurrentChainNet.forward, rnn_states being the actor's followed by the critic's.  Returns
        (mu [rows, A], value [rows, 1]).  keep=True: each engine's own heads buffer, and what backward() reads is kept;
        keep=False: views of `joint_heads`, and the next states - the actor's, then the critic's - in `last_states`."""
        n = self._states_each
        rows = x_raw.shape[0]
        a_args = self.actor.forward_pre_rnn(x_raw, rms, eps, tuple(rnn_states[:n]), dones, seq_length, keep)
        b_args = self.critic.forward_pre_rnn(x_raw, rms, eps, tuple(rnn_states[n:]), dones, seq_length, keep)
        self._sequence('forward', a_args, b_args, seq_length)
        mu_out = value_out = None
        if not keep:
            if self.joint_heads.shape[0] < rows:
                raise ValueError(f'{rows} rows in a step of a pair built for {self.joint_heads.shape[0]}')
            mu_out, value_out = self.joint_heads[:rows, 1:], self.joint_heads[:rows, :1]
        mu = self.actor.forward_post_rnn(keep, heads_out=mu_out)
        value = self.critic.forward_post_rnn(keep, heads_out=value_out)
        self.last_states = None if keep else tuple(self.actor.last_states) + tuple(self.critic.last_states)
        self._T = seq_length
        return mu, value

    @torch.no_grad()
    def backward(self):
        """d loss / d mu in actor.d_heads[:rows], d loss / d value in critic.d_heads[:rows] -> every gradient of the two
        trunks, RNNs, layer norms and heads in the arena (overwritten)."""
        a_args = self.actor.backward_pre_rnn()
        b_args = self.critic.backward_pre_rnn()
        self._sequence('backward', a_args, b_args, self._T)
        self.actor.backward_post_rnn()
        self.critic.backward_post_rnn()
