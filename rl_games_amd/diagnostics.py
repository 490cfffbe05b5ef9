"""PPO diagnostics (`use_diagnostics: True`, rl_games/common/diagnostics.py): the clip fraction of each mini-epoch, the
explained variance of the value targets and the running normaliser statistics, written to the summary writer once per
epoch.

The reference reduces every minibatch on the host (two `.cpu()` reads per optimiser step).  Here each minibatch is one
launch (ops.ppo_diag, csrc/ppo_diag.hip) inside the update - and inside its captured graphs - that writes the clip
columns of the minibatch's row of a device table: rows, mask sum, clipped count.  The explained variance needs only the
dataset's old values, returns and masks, which do not change while a mini-epoch trains on them: `mini_epoch` copies
the clip columns into the epoch's table and adds the centred moments of every minibatch slice with ONE launch
(ops.ppo_diag_moments) - at mini-epoch 0, later mini-epochs copy them unless the dataset is re-permuted - all on the
device; `epoch` reads that table once and forms the reference's numbers from it in
fp64 (fold_rows):

- explained variance (torch_ext.py:197-215), 1 - var(returns - values) / var(y): without masks population variances
  with y = returns; with masks the unbiased masked variances of get_mean_var_with_masks with y = the VALUES (y_pred);
  value_size V > 1: over the rows x V elements, the [rows, 1] mask broadcast over the columns as in the reference;
- clip fraction (torch_ext.py:217-227): without masks the minibatch mean; with masks the per-row tensor clip * m / sum(m),
  so that the mini-epoch mean is mean_i(C_i / M_i) / rows (a minibatch without valid rows gives NaN).
Both masked forms are the reference's behaviour, reproduced as it is."""
import torch

from . import ops

# columns of a table row (include/rlg_hip.h, rlg_ppo_diag / rlg_ppo_diag_moments)
ROWS, WEIGHT, CLIPPED, MEAN_RET, M2_RET, MEAN_VAL, M2_VAL, MEAN_DIFF, M2_DIFF, ELEMENTS = range(10)
STATS = 10


def reference_row(values, returns, new_neglogp, old_neglogp, e_clip, masks=None):
    """The table row of one minibatch as torch fp64 ops on the host (the kernels' contract; tests and CPU tensors use
    it).  values / returns [rows] or [rows, V]; neglogp and masks per row."""
    rows = old_neglogp.numel()
    values, returns = values.detach().reshape(-1).cpu(), returns.detach().reshape(-1).cpu()
    V = values.numel() // rows
    v, r = values.double(), returns.double()
    d = (returns.float() - values.float()).double()
    logratio = old_neglogp.detach().reshape(-1).float().cpu() - new_neglogp.detach().reshape(-1).float().cpu()
    lo, hi = ops.ppo_diag_log_bounds(e_clip)
    clipped = ((logratio < lo) | (logratio > hi)).double()
    m = torch.ones(rows, dtype=torch.float64) if masks is None else masks.detach().reshape(-1).double().cpu()
    me = m.repeat_interleave(V)
    we = me.sum()
    row = torch.zeros(STATS, dtype=torch.float64)
    row[ROWS], row[WEIGHT], row[CLIPPED], row[ELEMENTS] = rows, m.sum(), (clipped * m).sum(), values.numel()
    for k, x in ((MEAN_RET, r), (MEAN_VAL, v), (MEAN_DIFF, d)):
        mean = (x * me).sum() / we if we > 0 else torch.zeros((), dtype=torch.float64)
        row[k], row[k + 1] = mean, (me * (x - mean) ** 2).sum()
    return row


def _masked_var(mean, m2, w, V):
    """get_mean_var_with_masks (torch_ext.py:182-190) of a [rows, V] tensor under a [rows, 1] mask of row weight w, from
    the element-weighted centred moments (element weight V w): S = max(w, 1), min_sqr = sum (x m)^2 / S - (sum x m / S)^2,
    var = min_sqr S / max(S - 1, 1).  V = 1: M2 / max(w - 1, 1) directly (no cancellation)."""
    if bool((V == 1).all()):
        return m2 / torch.clamp(w - 1.0, min=1.0)
    S = torch.clamp(w, min=1.0)
    s1 = V * w * mean
    s2 = m2 + V * w * mean * mean
    return (s2 / S - (s1 / S) ** 2) * S / torch.clamp(S - 1.0, min=1.0)


def fold_rows(rows, masked):
    """(clip fraction, [explained variance per row]) of one mini-epoch's rows (fp64 [minibatches, STATS])."""
    rows = rows.double()
    n, w, c, e = rows[:, ROWS], rows[:, WEIGHT], rows[:, CLIPPED], rows[:, ELEMENTS]
    if masked:
        V = e / n
        var_y = _masked_var(rows[:, MEAN_VAL], rows[:, M2_VAL], w, V)
        var_dy = _masked_var(rows[:, MEAN_DIFF], rows[:, M2_DIFF], w, V)
        clip = (c / w).mean() / n[0]
    else:
        var_y, var_dy = rows[:, M2_RET] / e, rows[:, M2_DIFF] / e
        clip = (c / n).mean()
    return clip, 1.0 - var_dy / var_y


class DefaultDiagnostics:
    """Diagnostics off (or a rank other than 0): every method does nothing."""

    def send_info(self, writer):
        pass

    def epoch(self, agent, current_epoch):
        pass

    def mini_epoch(self, agent, miniepoch):
        pass

    def mini_batch(self, agent, batch, e_clip, minibatch):
        pass


class PpoDiagnostics(DefaultDiagnostics):
    def __init__(self):
        self.diag_dict = {}
        self.current_epoch = 0
        self.debug_neglogp = None   # [minibatches, rows] fp32 or None: receives each minibatch's new neglogp (tests)
        self._masked = False
        self._rows = None           # device [minibatches, STATS]: clip columns per minibatch slot, rewritten each mini-epoch
        self._table = None          # device [mini_epochs, minibatches, STATS]
        self._mini_epochs = []      # mini-epoch indices folded into _table this epoch, in order
        self._host_rows = {}        # minibatch slot -> CPU row (mini_batch with CPU tensors)
        self._host_table = []

    def allocate(self, mini_epochs, minibatches, minibatch_rows, device, value_size=1):
        """The device table and the launch scratch, allocated once - in front of any graph capture."""
        self._nmb, self._mb_rows = int(minibatches), int(minibatch_rows)
        self._rows = torch.zeros(self._nmb, STATS, dtype=torch.float64, device=device)
        self._table = torch.zeros(int(mini_epochs), self._nmb, STATS, dtype=torch.float64, device=device)
        self._partials = torch.zeros(ops.ppo_diag_blocks(self._mb_rows) * 3, dtype=torch.float64, device=device)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=device)
        mblocks = ops.ppo_diag_moments_blocks(self._mb_rows, value_size)
        self._moment_partials = torch.zeros(self._nmb * mblocks * 9, dtype=torch.float64, device=device)
        self._moment_tickets = torch.zeros(self._nmb, dtype=torch.int32, device=device)

    def mini_batch(self, agent, batch, e_clip, minibatch):
        """Row `minibatch` (the dataset slot) of the current mini-epoch.  batch: 'values', 'returns', 'old_neglogp',
        'masks' and either 'new_neglogp' or ('mu', 'logstd', 'actions') - the new neglogp recomputed on the device.
        Device tensors: one launch (the clip columns; the moments follow in mini_epoch), nothing read back; CPU tensors:
        the whole fp64 row on the host."""
        masks = batch.get('masks')
        self._masked = masks is not None
        old = batch['old_neglogp']
        if not old.is_cuda:
            self._host_rows[minibatch] = reference_row(batch['values'], batch['returns'], batch['new_neglogp'], old,
                                                       e_clip, masks)
            return
        if self._rows is None or minibatch >= self._nmb:
            raise RuntimeError('PpoDiagnostics.allocate() must size the table before the first minibatch')
        mb = old.numel()
        mask = None if masks is None else masks.reshape(-1).float().contiguous()
        nlp_out = None if self.debug_neglogp is None else self.debug_neglogp[minibatch, :mb]
        ops.ppo_diag(self._rows[minibatch], old.reshape(-1), e_clip, self._partials, self._ticket, mask=mask,
                     new_neglogp=batch.get('new_neglogp'), mu=batch.get('mu'), logstd=batch.get('logstd'),
                     actions=batch.get('actions'), neglogp_out=nlp_out)

    def mini_epoch(self, agent, miniepoch):
        """Folds the mini-epoch's rows into the epoch's table (device to device: no host synchronisation).  Mini-epoch 0
        starts a new epoch's table: an epoch that was never read by epoch() is dropped, not carried over."""
        if miniepoch == 0:
            self._mini_epochs, self._host_table = [], []
        if self._host_rows:
            self._host_table.append((miniepoch, torch.stack([self._host_rows[k] for k in sorted(self._host_rows)])))
            self._host_rows = {}
            return
        if self._table is None:
            return
        slot = len(self._mini_epochs)
        if slot >= self._table.shape[0]:
            raise RuntimeError('more mini-epochs in one epoch than the diagnostics table holds')
        t = self._table[slot]
        if slot > 0 and not getattr(agent.dataset, 'permute', False):
            # the same slices of the same old values / returns / masks as mini-epoch 0: its moments, copied on the device
            t.copy_(self._table[0])
            t[:, :CLIPPED + 1].copy_(self._rows[:, :CLIPPED + 1])
            self._mini_epochs.append(miniepoch)
            return
        t.copy_(self._rows)
        vd = agent.dataset.values_dict
        n = self._nmb * self._mb_rows
        masks = vd.get('rnn_masks')
        mask = None if masks is None else masks.reshape(-1)[:n].float().contiguous()
        def rows_of(x):                            # the minibatch slices' rows, all value columns
            return x.reshape(-1)[:n * (x.numel() // x.shape[0])]
        ops.ppo_diag_moments(t, rows_of(vd['old_values']), rows_of(vd['returns']), self._nmb, self._mb_rows,
                             self._moment_partials, self._moment_tickets, mask=mask)
        self._mini_epochs.append(miniepoch)

    def _epoch_tables(self):
        if self._host_table:
            out, self._host_table = self._host_table, []
            return out
        if not self._mini_epochs:
            return []
        table = self._table[:len(self._mini_epochs)].cpu()      # the one device-to-host read of the epoch
        out = list(zip(self._mini_epochs, table))
        self._mini_epochs = []
        return out

    def epoch(self, agent, current_epoch):
        self.current_epoch = current_epoch
        exp_vars = []
        for mini_ep, rows in self._epoch_tables():
            clip, ev = fold_rows(rows, self._masked)
            self.diag_dict[f'diagnostics/clip_frac/{mini_ep}'] = clip.float()
            exp_vars.append(ev)
        if agent.normalize_rms_advantage:
            adv_mean, adv_std = agent.advantage_mean_std.get_mean_std()
            self.diag_dict['diagnostics/rms_advantage/mean'] = adv_mean.detach()
            self.diag_dict['diagnostics/rms_advantage/var'] = (adv_std * adv_std).detach()
        if agent.normalize_value:
            self.diag_dict['diagnostics/rms_value/mean'] = agent.value_mean_std.running_mean
            self.diag_dict['diagnostics/rms_value/var'] = agent.value_mean_std.running_var
        if exp_vars:
            self.diag_dict['diagnostics/exp_var'] = torch.cat(exp_vars).mean().float()

    def send_info(self, writer):
        if writer is None:
            return
        for k, v in self.diag_dict.items():
            writer.add_scalar(k, v.cpu().numpy(), self.current_epoch)
