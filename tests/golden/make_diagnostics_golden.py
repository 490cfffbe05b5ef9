"""Generates tests/golden/epoch_diagnostics.pt from the REAL reference: one train_epoch of the reference agent with
`use_diagnostics: True`, then `diagnostics.epoch(agent, 1)` (what train() calls), recorded through make_golden's
recorders (make_epoch / make_discrete: rollout, initial state, per-minibatch losses) plus every `mini_batch` call's
tensors and the final `diag_dict`.

Run in the build container only (needs the reference checkout):

    python tests/golden/make_diagnostics_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
import ref_import  # noqa: E402

FILENAME = 'epoch_diagnostics.pt'


def _record(make, variants, tmp_name):
    """Run one make_golden recorder with every PpoDiagnostics of the reference recording its calls; returns
    {variant: capture + 'diag'}."""
    ref_import.enable()
    from rl_games.common import diagnostics as ref_diag
    calls = []          # one entry per agent, in the order the recorder builds them
    orig_init, orig_mb = ref_diag.PpoDiagnostics.__init__, ref_diag.PpoDiagnostics.mini_batch

    def init(self):
        orig_init(self)
        calls.append({'obj': self, 'agent': None, 'minibatches': []})

    def mini_batch(self, agent, batch, e_clip, minibatch):
        rec = next(c for c in calls if c['obj'] is self)
        rec['agent'] = agent
        rec['minibatches'].append({k: (None if v is None else v.detach().clone()) for k, v in batch.items()}
                                  | {'e_clip': float(e_clip)})
        return orig_mb(self, agent, batch, e_clip, minibatch)

    ref_diag.PpoDiagnostics.__init__, ref_diag.PpoDiagnostics.mini_batch = init, mini_batch
    try:
        make(variants, tmp_name)
    finally:
        ref_diag.PpoDiagnostics.__init__, ref_diag.PpoDiagnostics.mini_batch = orig_init, orig_mb
    path = os.path.join(HERE, tmp_name)
    caps = torch.load(path, weights_only=False)
    os.remove(path)
    assert len(calls) == len(caps)
    for (name, cap), rec in zip(caps.items(), calls):
        d, agent = rec['obj'], rec['agent']
        d.epoch(agent, current_epoch=1)
        cap['diag'] = {'minibatches': rec['minibatches'], 'mini_epochs': agent.mini_epochs_num,
                       'diag_dict': {k: v.detach().clone() for k, v in d.diag_dict.items()},
                       'e_clip': float(agent.e_clip)}
    return caps


def main():
    out = {}
    out.update(_record(make_golden.make_epoch, {
        'default': dict(use_diagnostics=True),
        'smooth_reg_ema': dict(use_diagnostics=True, use_smooth_clamp=True, bound_loss_type='regularisation',
                               bounds_loss_coef=0.01, normalize_rms_advantage=True, entropy_coef=0.01, critic_coef=1.0),
        'lstm': dict(use_diagnostics=True, seq_length=4, _rnn={'name': 'lstm', 'units': 16, 'layers': 1}),
    }, '_diag_continuous.pt'))
    discrete = _record(make_golden.make_discrete, {
        # next_step autoreset: masked filler rows (rnn_masks) - the masked explained-variance / clip-fraction forms
        'discrete_masked': dict(use_diagnostics=True, normalize_input=True, normalize_value=True, p_done=0.15),
        'multi_discrete_masked': dict(use_diagnostics=True, _autoreset='same_step', _heads=[3, 4], _masks=True,
                                      entropy_coef=0.02, p_done=0.05, normalize_input=True),
    }, '_diag_discrete.pt')
    for cap in discrete.values():
        cap['discrete'] = True
    out.update(discrete)
    torch.save(out, os.path.join(HERE, FILENAME))
    for name, cap in out.items():
        print(name, len(cap['diag']['minibatches']), 'minibatches',
              {k: round(float(v.reshape(-1)[0]), 6) for k, v in cap['diag']['diag_dict'].items()})
    print(FILENAME, 'written', os.path.getsize(os.path.join(HERE, FILENAME)) // 1024, 'KiB')


if __name__ == '__main__':
    main()
