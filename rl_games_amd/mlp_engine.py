"""Manual forward/backward of the actor-critic MLP (no autograd graph).

For the plain-MLP policies of the BASELINE configs the training step is a fixed chain
    obs -> [Linear -> act] x L -> fused (value | mu) head -> fused PPO loss kernel
so the backward pass is written out explicitly instead of being recorded by autograd:
  * the GEMMs are the same rocBLAS/hipBLASLt calls nn.Linear's autograd issues
    (forward addmm; dX = dZ W; dW = dZ^T A), written straight into preallocated buffers and
    into the gradient arena (no AccumulateGrad adds, no per-step allocations);
  * activation backward + bias-gradient column sum is ONE pass (csrc/mlp_fused.hip) instead of
    aten's elu_backward followed by a separate sum(0) reduction;
  * the value and mu heads (`a2c_network.value`, `a2c_network.mu`,
    rl_games/algos_torch/network_builder.py:295-311) are adjacent in the parameter arena and
    run as one [1+A, K] GEMM operand; their bias gradients come out of the loss kernel.
  * an optional single-layer LSTM between the trunk and the heads (BASELINE config #5,
    `rnn: {name: lstm, layers: 1}`, network_builder.py:447-512) runs as ONE sequence-persistent
    kernel per direction (csrc/lstm.hip; 128 units: csrc/lstm_wide.hip) instead of a Python loop of per-timestep MIOpen calls
    with done resets (rl_games/common/layers/recurrent.py:26-58) and autograd BPTT through it;
    its input projection and all four weight/bias gradients are whole-sequence GEMMs.
  * a single-layer GRU in that position (`rnn: {name: gru, layers: 1}`, network_builder.py:250-276) likewise
    (csrc/gru.hip; 128 units: csrc/gru_wide.hip): one state tensor instead of two, 3H gate columns, b_hh added inside
    the kernel, and a backward that emits the gradient of the input side (W_ih, b_ih, the trunk) and of the hidden
    side (W_hh, b_hh) as two arrays for the same weight-gradient and column-sum launches.
Numerics: aten's formulas - by default (in-place activations) act' from the layer output like
elu_backward(is_result=True): h > 0 ? 1 : h + 1; with `inplace_act=False` from the pre-activation
(exp(z)); GEMM
results are the library's, as before.  Parameters keep their reference names and shapes.
The recurrent cell's stations - its buffers, gate bias, ping-pong states, the sequence kernels' arguments, the gate
gradients' column sums and weight-gradient jobs - are chain_net.RnnStations, the same object RecurrentChainNet runs on;
this engine keeps its two trunk modes in front of it (the fused `chain_rnn`, or per-layer library products) and its own
head stations behind it.
backward() ends in chain_net.WeightGrads.finish - the one finisher of weight gradients, bias column sums and loss
partials that the chain engines use as well - here with the narrow kernel for left-over products and, on the fused
chain, the gradient norm and the fp16 form of the MFMA launch.
"""
import torch
from torch import nn

from . import ops
from .chain_net import RnnStations, WeightGrads, arena_layout, head_span, plain_trunk, trunk_jobs, trunk_views


class ManualMLP:
    def __init__(self, net, arena, max_rows, mfma_dw=True, inplace_act=True, fused_chain=True):
        """net: policy.ActorCriticNetwork (no RNN); arena: FlatArena laid out by `layout(net)`.
        mfma_dw: weight gradients through the one-launch f32-MFMA kernel (csrc/mlp_dw.hip).
        fused_chain: the whole MLP (observation normaliser, hidden layers, fused value|mu head) as
        ONE forward launch and ONE backward launch with the activations of a row tile resident in
        LDS (csrc/mlp_chain.hip); plain MLP policies only (the LSTM path keeps the per-layer GEMMs).
        (Measured and rejected: forking the library dW GEMMs onto a second stream - multi-branch
        hipGraphs cost more in cross-branch dependencies than the overlap gains.)"""
        self.net = net
        # a left-over product over a few observations (config #5: obs 3) on the narrow kernel, not the library
        self.weight_grads = WeightGrads(mfma=mfma_dw, narrow=True)
        self._x_normalised = False
        self.arena = arena
        self.linears, self.act_name = plain_trunk(net.actor_mlp)
        self.act_kind = ops.ACT_KINDS[self.act_name]
        if not isinstance(net.value_act, nn.Identity) or not isinstance(net.mu_act, nn.Identity):
            raise NotImplementedError('head activations are not supported by the manual MLP engine')
        self.A = net.mu.out_features
        self.V = net.value.out_features
        K = net.mu.in_features
        self.head_w, self.head_w_grad, self.head_b, self.head_b_grad, _ = head_span([net.value, net.mu], arena)
        self._head_mfma = (mfma_dw and self.V + self.A <= 64 and ops.mlp_rowgemm_supported(K, K)
                           and self.head_w.data_ptr() % 16 == 0)
        dev = self.head_w.device
        self.max_rows = max_rows
        # the recurrent cell between the trunk and the heads: chain_net.RnnStations, the one RecurrentChainNet runs on
        self.stations = RnnStations(net.rnn.rnn, max_rows, dev) if getattr(net, 'has_rnn', False) else None
        st = self.stations
        # the cell's torch module (parameters only): by kind, and whichever of the two it is
        self.lstm, self.gru, self.rnn = (st.lstm, st.gru, st.rnn) if st is not None else (None, None, None)
        widths = [l.out_features for l in self.linears]
        # inplace_act: the activation overwrites the pre-activation (one [rows, width] buffer per
        # layer instead of two) and backward takes act' from the output, like torch's in-place ELU
        # (elu_backward(is_result=True): h > 0 ? 1 : h + 1).  Halves the activation footprint of a
        # minibatch (276 -> 184 MB at 32,768 rows), which then fits the 256 MB Infinity Cache together
        # with the gradients.
        self.inplace_act = bool(inplace_act) and self.act_kind in (1, 2, 3)
        self.Hs = [torch.empty(max_rows, w, device=dev) for w in widths]      # activations
        self.Z = self.Hs if (self.inplace_act or self.act_kind == 0) else \
            [torch.empty(max_rows, w, device=dev) for w in widths]            # pre-activations
        self.dA = [torch.empty(max_rows, w, device=dev) for w in widths]      # d activation / d pre-act
        self.heads = torch.empty(max_rows, self.V + self.A, device=dev)
        self.d_heads = torch.empty(max_rows, self.V + self.A, device=dev)
        self.nb = [ops.act_bwd_blocks(max_rows, w) for w in widths]
        self.chain = None
        self._deferred = None            # arguments of a training forward that backward() will launch (forward_obs(defer=True))
        self.last_step_fused = False     # the last backward() ran forward + loss + backward as one launch
        self._pending_backward = False
        self._fused_trunk = False
        if fused_chain and self.rnn is None:
            try:
                layers = [(l.weight, l.bias, self.act_name) for l in self.linears]
                layers.append((self.head_w, self.head_b, 'None'))
                self.chain = ops.MlpChain(layers, dev, weights_version=arena.weights_token)
            except NotImplementedError:
                self.chain = None
        # Recurrent policies (round 3): the trunk IN FRONT of the LSTM - observation normaliser, hidden layers and
        # the gate-input product W_ih x + (b_ih + b_hh) as the chain's last (linear) layer - is the same fused
        # forward / backward launch pair; the sequence-persistent LSTM kernels and the head product follow.
        self.chain_rnn = None
        if fused_chain and self.rnn is not None:
            try:
                layers = [(l.weight, l.bias, self.act_name) for l in self.linears]
                layers.append((self.rnn.weight_ih_l0, st.gate_bias, 'None'))
                self.chain_rnn = ops.MlpChain(layers, dev, weights_version=arena.weights_token)
            except NotImplementedError:
                self.chain_rnn = None
        if self.chain is not None or self.chain_rnn is not None:
            self.nb = [(max_rows + 15) // 16 for _ in widths]      # one partial row per 16-row group at most
            self.xn = torch.empty(max_rows, self.linears[0].in_features, device=dev)
        self.partials = [torch.empty(nb * w, dtype=torch.float64, device=dev) for nb, w in zip(self.nb, widths)]

    # what the last backward()'s weight gradients ran on (bench.py and the tests read these)
    last_dw_path = property(lambda self: self.weight_grads.last_dw_path)
    last_dw_jobs = property(lambda self: self.weight_grads.last_dw_jobs)
    last_dw_library_jobs = property(lambda self: self.weight_grads.last_dw_library_jobs)
    # final states of the last keep=False forward of a recurrent policy
    last_states = property(lambda self: self.stations.last_states)

    @staticmethod
    def layout(net):
        """Physical arena order: every weight MATRIX first (parameters() order, the value and mu
        head weights last and adjacent), then the vectors (biases, sigma; value and mu head biases
        last and adjacent).  Matrix sizes are multiples of 4 floats for every supported shape, so
        all weight / weight-gradient views stay 16-byte aligned (vector loads/stores of the MFMA
        kernels); the logical (optimizer-state) order is untouched.  The layers' bias vectors come directly behind
        the last matrix (chain_net.arena_layout explains)."""
        linear_biases = [m.bias for m in net.modules() if isinstance(m, nn.Linear) and m.bias is not None]
        return arena_layout(list(net.parameters()), [[net.value, net.mu]], first_vectors=linear_biases)

    # ------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, keep=True, rnn_states=None, dones=None, seq_length=1, raw_rms=None, eps=1e-5):
        """x: [rows, in] normalised observations.  Returns heads [rows, V+A] (col 0..V-1 value,
        then mu).  `keep` retains what backward() needs (activations, LSTM cell states).  LSTM policies: rows are
        ordered (sequence, t) with `seq_length` steps each, rnn_states = (h0, c0) - GRU: (h0,) - of shape
        [1, rows/seq_length, H], dones [rows] u8 resets the state entering a step (or None);
        the final states are left in `self.last_states`.
        raw_rms (recurrent policies on the fused trunk, `chain_rnn`): x holds RAW observations and raw_rms =
        (running_mean, running_var) or () for normalize_input off - the launch normalises on the way in."""
        rows = x.shape[0]
        if self._pending_backward and not keep:
            # in-place activations: an inference forward reuses the buffers backward() reads
            raise RuntimeError('ManualMLP.forward(keep=False) would overwrite the activations a pending '
                               'backward() still needs')
        self._pending_backward = bool(keep)
        a = x
        fused_trunk = raw_rms is not None
        if fused_trunk and (self.chain_rnn is None or self.rnn is None):
            raise ValueError('raw_rms: the fused recurrent trunk is not available for this policy')
        for l, lin in enumerate(() if fused_trunk else self.linears):
            z = self.Z[l][:rows]
            torch.addmm(lin.bias, a, lin.weight.t(), out=z)
            h = self.Hs[l][:rows]                      # same storage as z when inplace_act
            if self.act_kind == 1:
                torch.ops.aten.elu.out(z, out=h)
            elif self.act_kind == 2:
                torch.clamp_min(z, 0.0, out=h)
            elif self.act_kind == 3:
                torch.tanh(z, out=h)
            else:
                h = z
            a = h
        if self.rnn is not None:
            st = self.stations
            args = st.forward_args(rows, rnn_states, dones, seq_length, keep)
            gates = args[0]
            if fused_trunk:
                rms = raw_rms if len(raw_rms) else None
                if keep:
                    acts = [h[:rows] for h in self.Hs]
                    xn = self.xn[:rows] if rms is not None else None
                    self.chain_rnn.forward(x, gates, act_out=acts, rms=rms, eps=eps, xn_out=xn)
                    x = xn if rms is not None else x          # what the first layer's weight gradient reads
                    a = acts[-1]
                else:
                    self.chain_rnn.forward(x, gates, rms=rms, eps=eps)
                    a = None
            else:
                torch.addmm(st.gate_bias, a, self.rnn.weight_ih_l0.t(), out=gates)
            st.sequence('forward', args, seq_length)
            self._rnn_in = a
            a = st.rnn_out[:rows]
        heads = self.heads[:rows]
        if self._head_mfma and a.is_contiguous() and a.data_ptr() % 16 == 0:
            # skinny output (1 + A columns): the LDS-free MFMA kernel beats the library GEMM 2.5x here
            # (8 vs 20 us at 32,768 x 100 -> 22); for the wide hidden layers the library stays ahead.
            ops.mlp_linear_act_forward(a, self.head_w, self.head_b, heads, act_kind=0)
        else:
            torch.addmm(self.head_b, a, self.head_w.t(), out=heads)
        self._x, self._rows, self._last = x, rows, a
        self._fused_trunk = fused_trunk and keep
        return heads

    @torch.no_grad()
    def forward_obs(self, obs, rms=None, eps=1e-5, keep=True, rms_fold=None, defer=False):
        """Fused chain: obs [rows, in] RAW observations; rms = (running_mean, running_var) fp64 or None
        (normalize_input off).  One launch: normalise -> hidden layers -> heads.  keep=True retains
        the activations and the normalised observations for backward(); keep=False (rollout,
        get_values) writes nothing but the heads, so it cannot disturb a pending backward.
        rms_fold: RunningMeanStd.fold_buffers() - the statistics update of a training forward happens
        in the launch's prologue.  defer=True (training forward whose backward() follows with a ppo_loss descriptor):
        nothing is launched yet - backward() issues forward + loss + backward as ONE launch where the chain has that
        form (ops.MlpChain.step: minibatches < 16,384 rows), else the forward now-deferred and then the backward; the
        returned heads view is where the values will be."""
        rows = obs.shape[0]
        heads = self.heads[:rows]
        self._deferred = None
        if keep:
            acts = [h[:rows] for h in self.Hs]
            xn = self.xn[:rows] if rms is not None else None
            if defer:
                self._deferred = dict(x=obs, heads=heads, act_out=acts, rms=rms, eps=eps, xn_out=xn, rms_fold=rms_fold)
            else:
                self.chain.forward(obs, heads, act_out=acts, rms=rms, eps=eps, xn_out=xn, rms_fold=rms_fold)
            self._x = xn if rms is not None else obs
            self._x_normalised = rms is not None          # (went through the normaliser's clamp to [-5, 5])
            self._rows, self._last = rows, acts[-1]
            self._pending_backward = True
        else:
            self.chain.forward(obs, heads, rms=rms, eps=eps)
        return heads

    def _one_launch_step(self, fwd, d_heads, dzs, parts, ppo_loss):
        ok = self.chain.step(fwd['x'], fwd['heads'], fwd['act_out'], d_heads, dzs, parts, ppo_loss, rms=fwd['rms'],
                             eps=fwd['eps'], xn_out=fwd['xn_out'], rms_fold=fwd['rms_fold'])
        self.last_step_fused = bool(ok)
        return ok

    def gradient_elements(self):
        """Number of arena gradient elements that backward() + the loss finalise produce on the fused
        path: trunk weights and biases, the fused head matrix, the head biases and logstd."""
        n = sum(l.weight.numel() + l.bias.numel() for l in self.linears)
        return n + self.head_w_grad.numel() + (self.V + self.A) + self.A

    def values_view(self, heads):
        return heads[:, :self.V]

    def mu_view(self, heads):
        return heads[:, self.V:]

    @torch.no_grad()
    def backward(self, d_heads, loss_finalize=None, norm=None, ppo_loss=None):
        """d_heads [rows, V+A] = d loss / d heads.  Writes every weight/bias gradient of the trunk
        and the head WEIGHT gradient into the arena (head bias gradients are written by the loss
        finalise kernel).  The dX chain runs first; the weight gradients - which nothing in that
        chain waits for - are then ONE f32-MFMA launch for all layers (csrc/mlp_dw.hip), or the
        library GEMMs when a shape is outside that kernel's envelope / `mfma_dw` is off.
        loss_finalize: ops.loss_finalize_desc(...) - folded in the weight-gradient finalise launch when
        there is one, launched on its own otherwise.  norm = (partials, grad_scale, step_counter): see
        ops.MlpDwPlan.launch; returns the number of valid norm partials, or None when the gradient norm
        was not produced (a gradient of this step did not come out of that launch).  ppo_loss
        (ops.ppo_loss_desc, fused chain only): the backward launch evaluates the PPO loss first and so
        produces d_heads itself."""
        rows = self._rows
        L = len(self.linears)
        self._pending_backward = False
        if self.chain is not None:
            # one launch: dZ of every hidden layer + per-workgroup bias-gradient column sums
            nblk = self.chain.num_blocks(rows, 1)
            acts, dzs, parts = trunk_views(self.linears, self.Hs, self.dA, self.partials, rows, nblk)
            fwd, self._deferred = self._deferred, None
            self.last_step_fused = False
            if fwd is None or not (ppo_loss is not None and self._one_launch_step(fwd, d_heads, dzs, parts, ppo_loss)):
                if fwd is not None:                     # (no one-launch form for this shape: the two launches)
                    self.chain.forward(fwd['x'], fwd['heads'], act_out=fwd['act_out'], rms=fwd['rms'], eps=fwd['eps'],
                                       xn_out=fwd['xn_out'], rms_fold=fwd['rms_fold'])
                self.chain.backward(d_heads, acts, dzs, parts, ppo_loss=ppo_loss)
            # (dZ, X, grad, layer): the layer index names dZ's row of the backward's gradient maxima (fp16 form)
            jobs, colsums = trunk_jobs(self.linears, self._x, acts, dzs, parts, nblk)
            jobs.insert(0, (d_heads, acts[-1], self.head_w_grad, L))
            # the fp16 form of the weight-gradient launch splits X under the forward's FIXED scales: hidden activations, and
            # observations that went through the normaliser's clamp (raw observations have no bound: the bf16 form then)
            maxima = self.chain.gradient_maxima(rows) if self._x_normalised else None
            if maxima is not None:
                maxima = (maxima, self.chain.maxima_rows_per_entry)
            return self.weight_grads.finish(jobs, rows, colsums, loss_finalize, norm, maxima=maxima)
        jobs = [(d_heads, self._last, self.head_w_grad)]           # (dZ, X, grad) per weight matrix
        colsums = []                                               # (partials, blocks, cols, bias.grad)
        if self.rnn is not None:
            st = self.stations
            d_out = st.d_rnn_out[:rows]
            if self.V + self.A <= ops.NARROW_MAX:
                ops.narrow_dx(d_heads, self.head_w, d_out)
            else:
                torch.mm(d_heads, self.head_w, out=d_out)
            st.sequence('backward', st.backward_args(d_out), st.seq_length)
            dg, gate_jobs, colsums = st.gate_gradients(self._rnn_in)
            jobs += gate_jobs
            if self._fused_trunk:
                # dX chain of the trunk in ONE launch, from d gates down: dZ of every hidden layer + the
                # per-workgroup bias-gradient column sums (the chain's "head" layer is W_ih)
                nblk = self.chain_rnn.num_blocks(rows, 1)
                acts, dzs, parts = trunk_views(self.linears, self.Hs, self.dA, self.partials, rows, nblk)
                self.chain_rnn.backward(dg, acts, dzs, parts)
                trunk, trunk_colsums = trunk_jobs(self.linears, self._x, acts, dzs, parts, nblk)
                return self.weight_grads.finish(jobs + trunk, rows, colsums + trunk_colsums, loss_finalize)
            d = self.dA[L - 1][:rows]
            torch.mm(dg, self.rnn.weight_ih_l0, out=d)
        else:
            d = self.dA[L - 1][:rows]
            torch.mm(d_heads, self.head_w, out=d)
        for l in range(L - 1, -1, -1):
            lin = self.linears[l]
            w = lin.out_features
            nb = ops.act_bwd_blocks(rows, w)
            part = self.partials[l][:nb * w]
            ops.act_bwd_colsum(d, self.Z[l][:rows], d, self.act_kind + (16 if self.inplace_act else 0), part, nb)
            colsums.append((part, nb, w, lin.bias.grad))
            a_prev = self.Hs[l - 1][:rows] if l > 0 else self._x
            jobs.append((d, a_prev, lin.weight.grad))
            if l > 0:
                d_prev = self.dA[l - 1][:rows]
                torch.mm(d, lin.weight, out=d_prev)
                d = d_prev
        return self.weight_grads.finish(jobs, rows, colsums, loss_finalize)
