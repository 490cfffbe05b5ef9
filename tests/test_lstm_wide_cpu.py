"""CPU: the 128-unit LSTM configuration (configs.pendulum_lstm_4096(units=128)) and the boundary of its kernels."""
import pytest
import torch


# BASELINE.json config #5 as configs.pendulum_lstm_4096() returned it before the `units` keyword existed
_CONFIG5 = {
    'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'},
    'network': {
        'name': 'actor_critic', 'separate': False,
        'space': {'continuous': {
            'mu_activation': 'None', 'sigma_activation': 'None',
            'mu_init': {'name': 'default'},
            'sigma_init': {'name': 'const_initializer', 'val': 0},
            'fixed_sigma': True}},
        'mlp': {'units': [64, 64], 'activation': 'elu', 'initializer': {'name': 'default'}},
        'rnn': {'name': 'lstm', 'units': 64, 'layers': 1},
    },
    'config': {
        'name': 'pendulum_lstm', 'env_name': 'synthetic', 'env_config': {'obs_dim': 3, 'act_dim': 1},
        'normalize_input': True, 'normalize_value': True, 'normalize_advantage': True,
        'value_bootstrap': True, 'reward_shaper': {'scale_value': 1.0},
        'gamma': 0.99, 'tau': 0.95, 'learning_rate': 3e-4, 'lr_schedule': 'adaptive',
        'kl_threshold': 0.008, 'grad_norm': 1.0, 'entropy_coef': 0.0, 'truncate_grads': True,
        'e_clip': 0.2, 'clip_value': True, 'critic_coef': 2, 'bounds_loss_coef': 1e-4,
        'bound_loss_type': 'bound', 'num_actors': 4096, 'horizon_length': 16,
        'minibatch_size': 16384, 'mini_epochs': 4, 'max_epochs': -1,
        'mixed_precision': False, 'print_stats': False, 'save_frequency': 0,
        'save_best_after': 10 ** 9, 'device': 'cuda:0', 'multi_gpu': False,
        'train_dir': '/tmp/rl_games_amd_runs', 'seq_length': 16,
    },
}


def _same(a, b):
    """Deep equality that also tells 2 from 2.0 and a list from a tuple."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_config5_is_unchanged():
    from rl_games_amd import configs
    assert _same(configs.pendulum_lstm_4096(), _CONFIG5)
    assert _same(configs.pendulum_lstm_4096(units=64), _CONFIG5)


def test_wide_config_differs_in_units_only():
    from rl_games_amd import configs
    import copy
    wide = configs.pendulum_lstm_4096(units=128)
    assert wide['network']['rnn']['units'] == 128
    want = copy.deepcopy(_CONFIG5)
    want['network']['rnn']['units'] = 128
    assert _same(wide, want)
    # overrides still reach the config section, and `units` does not leak into it
    small = configs.pendulum_lstm_4096(num_actors=128, units=128, minibatch_size=1024)
    assert small['config']['num_actors'] == 128 and small['config']['minibatch_size'] == 1024
    assert 'units' not in small['config']


def test_wide_lstm_ops_reject_cpu_tensors():
    from rl_games_amd import ops
    from rl_games_amd._lib import HipLibraryError
    S, T, H = 4, 2, 128
    gates = torch.zeros(S * T, 4 * H)
    w_hh = torch.zeros(4 * H, H)
    state = torch.zeros(S, H)
    rows = torch.zeros(S * T, H)
    with pytest.raises(HipLibraryError):
        ops.lstm_seq_forward(gates, w_hh, state, state, None, rows, seq_len=T)
    with pytest.raises(HipLibraryError):
        ops.lstm_seq_backward(gates, rows, state, None, w_hh, rows, torch.zeros(S * T, 4 * H), T)


def test_lstm_ops_reject_rows_that_are_no_multiple_of_seq_len():
    from rl_games_amd import ops
    H = 16
    gates = torch.zeros(7, 4 * H)
    w_hh = torch.zeros(4 * H, H)
    state = torch.zeros(3, H)
    rows = torch.zeros(7, H)
    with pytest.raises(ValueError, match='multiple of seq_len'):
        ops.lstm_seq_forward(gates, w_hh, state, state, None, rows, seq_len=2)
    with pytest.raises(ValueError, match='multiple of seq_len'):
        ops.lstm_seq_backward(gates, rows, state, None, w_hh, rows, torch.zeros(7, 4 * H), 2)
