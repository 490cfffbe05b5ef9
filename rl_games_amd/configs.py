"""Parameter dictionaries for the BASELINE.json configurations (synthetic, device-resident
environments of the named shapes).  Hyper-parameters follow SURVEY 8(d) / BASELINE.md 3 (they
mirror rl_games/configs/mujoco/ant.yaml:36-57): adaptive lr, kl_threshold 0.008, e_clip 0.2,
clip_value, critic_coef 2, normalize input/value/advantage, truncate_grads, fp32."""
import copy


def _network(units, rnn=None):
    net = {
        'name': 'actor_critic', 'separate': False,
        'space': {'continuous': {
            'mu_activation': 'None', 'sigma_activation': 'None',
            'mu_init': {'name': 'default'},
            'sigma_init': {'name': 'const_initializer', 'val': 0},
            'fixed_sigma': True}},
        'mlp': {'units': list(units), 'activation': 'elu', 'initializer': {'name': 'default'}},
    }
    if rnn is not None:
        net['rnn'] = dict(rnn)
    return net


def _config(name, num_actors, horizon, minibatch, mini_epochs, env_config, **over):
    cfg = {
        'name': name, 'env_name': 'synthetic', 'env_config': dict(env_config),
        'normalize_input': True, 'normalize_value': True, 'normalize_advantage': True,
        'value_bootstrap': True, 'reward_shaper': {'scale_value': 1.0},
        'gamma': 0.99, 'tau': 0.95, 'learning_rate': 3e-4, 'lr_schedule': 'adaptive',
        'kl_threshold': 0.008, 'grad_norm': 1.0, 'entropy_coef': 0.0, 'truncate_grads': True,
        'e_clip': 0.2, 'clip_value': True, 'critic_coef': 2, 'bounds_loss_coef': 1e-4,
        'bound_loss_type': 'bound', 'num_actors': num_actors, 'horizon_length': horizon,
        'minibatch_size': minibatch, 'mini_epochs': mini_epochs, 'max_epochs': -1,
        'mixed_precision': False, 'print_stats': False, 'save_frequency': 0,
        'save_best_after': 10 ** 9, 'device': 'cuda:0', 'multi_gpu': False,
        'train_dir': '/tmp/rl_games_amd_runs',
    }
    cfg.update(over)
    return cfg


def humanoid_65536(num_actors=65536, minibatch_size=32768, **over):
    """BASELINE.json config #3/#4: Isaac-Humanoid-shaped obs 108 / act 21, 65,536 x 32."""
    return {'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'},
            'network': _network([400, 200, 100]),
            'config': _config('humanoid_shaped', num_actors, 32, minibatch_size, 5,
                              {'obs_dim': 108, 'act_dim': 21}, **over)}


def ant_4096(num_actors=4096, **over):
    """BASELINE.json config #2: Ant-v5-shaped obs 60 / act 8, 4,096 x 16."""
    return {'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'},
            'network': _network([256, 128, 64]),
            'config': _config('ant_shaped', num_actors, 16, min(32768, num_actors * 16), 4,
                              {'obs_dim': 60, 'act_dim': 8}, **over)}


def pendulum_lstm_4096(num_actors=4096, units=64, **over):
    """BASELINE.json config #5: LSTM policy, Pendulum-shaped obs 3 / act 1, 4,096 x seq_len 16.
    units: width of the LSTM (config #5 itself: 64; 128 is the width of the reference's ppo_continuous_lstm.yaml)."""
    return {'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'},
            'network': _network([64, 64], rnn={'name': 'lstm', 'units': units, 'layers': 1}),
            'config': _config('pendulum_lstm', num_actors, 16, min(16384, num_actors * 16), 4,
                              {'obs_dim': 3, 'act_dim': 1}, seq_length=16, **over)}


def pendulum_gru_4096(num_actors=4096, units=64, **over):
    """Config #5's shape with a GRU in the LSTM's place (`rnn: {name: gru, layers: 1}`; 128 units is the cell of the
    reference's configs/smac/v1/runs/MMM2_rnn.yaml).  Everything but the cell's name is pendulum_lstm_4096's."""
    params = pendulum_lstm_4096(num_actors=num_actors, units=units, **over)
    params['network']['rnn']['name'] = 'gru'
    return params


def lunar_separate_rnn(num_actors=16, units=64, cell='lstm', layer_norm=False, **over):
    """The reference's continuous recurrent configurations (rl_games/configs/ppo_lunar_continiuos_torch.yaml and, with
    `layer_norm=True`, the network of configs/test/test_asymmetric_continuous.yaml): separate actor / critic trunks
    [64] relu, each with its own LSTM layer of 64 units, LunarLanderContinuous-shaped obs 8 / act 2, 16 actors x 128
    steps in sequences of 4.  Hyper-parameters follow ppo_lunar_continiuos_torch.yaml."""
    net = _network([64], rnn={'name': cell, 'units': units, 'layers': 1, 'layer_norm': bool(layer_norm)})
    net['separate'] = True
    net['mlp']['activation'] = 'relu'
    horizon = over.pop('horizon_length', 128)
    cfg = _config('lunar_separate_rnn', num_actors, horizon, over.pop('minibatch_size', num_actors * horizon // 2), 4,
                  {'obs_dim': 8, 'act_dim': 2}, normalize_value=False, value_bootstrap=False, tau=0.9,
                  learning_rate=1e-3, grad_norm=0.5, critic_coef=1, bounds_loss_coef=0, seq_length=4,
                  reward_shaper={'scale_value': 0.1})
    cfg.update(over)
    return {'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'}, 'network': net,
            'config': cfg}


def tiny(num_actors=256, horizon=8, obs_dim=12, act_dim=3, **over):
    """Small config for smoke tests."""
    return {'algo': {'name': 'a2c_continuous'}, 'model': {'name': 'continuous_a2c_logstd'},
            'network': _network([32, 16]),
            'config': _config('tiny', num_actors, horizon, num_actors * horizon // 2, 2,
                              {'obs_dim': obs_dim, 'act_dim': act_dim}, **over)}


def cartpole_discrete(num_actors=16, **over):
    """BASELINE.json config #1 (rl_games/configs/ppo_cartpole.yaml): discrete PPO, CartPole-shaped
    obs 4 / 2 actions, separate actor/critic MLPs [32,32] relu, next_step autoreset (masked rows)."""
    net = {'name': 'actor_critic', 'separate': True, 'space': {'discrete': None},
           'mlp': {'units': [32, 32], 'activation': 'relu', 'initializer': {'name': 'default'}}}
    cfg = _config('cartpole_shaped', num_actors, 32, 64, 4,
                  {'obs_dim': 4, 'discrete_actions': 2, 'autoreset_mode': 'next_step'},
                  normalize_input=False, normalize_value=False, learning_rate=2e-4, lr_schedule=None,
                  entropy_coef=0.01, critic_coef=1, tau=0.9, reward_shaper={'scale_value': 0.1})
    cfg.pop('bounds_loss_coef')
    cfg.pop('bound_loss_type')
    cfg.update(over)
    return {'algo': {'name': 'a2c_discrete'}, 'model': {'name': 'discrete_a2c'}, 'network': net, 'config': cfg}


def smac_rnn_discrete(num_actors=8, cell='lstm', units=128, layer_norm=False, actions=14, **over):
    """The shape of the reference's recurrent SMAC runs (rl_games/configs/smac/v1/runs/MMM2_rnn.yaml, 6h_vs_8z_rnn.yaml;
    `layer_norm: True` as in 5m_vs_6m_rnn.yaml): discrete PPO, a shared ReLU trunk, one LSTM / GRU layer of `units`
    behind it, action masks, sequences of 8 steps, normalised observations and values - on the synthetic env (obs 80;
    `actions`: an int for Discrete, a list for multi-discrete heads).  Hyper-parameters follow MMM2_rnn.yaml."""
    multi = isinstance(actions, (list, tuple))
    net = {'name': 'actor_critic', 'separate': False, 'space': {'multi_discrete' if multi else 'discrete': None},
           'mlp': {'units': [256, 128], 'activation': 'relu', 'initializer': {'name': 'default'}},
           'rnn': {'name': cell, 'units': units, 'layers': 1, 'layer_norm': bool(layer_norm)}}
    horizon = over.pop('horizon_length', 32)
    minibatch = over.pop('minibatch_size', max(num_actors * horizon // 2, 8))
    cfg = _config('smac_rnn_shaped', num_actors, horizon, minibatch, 4,
                  {'obs_dim': 80, 'discrete_actions': list(actions) if multi else int(actions), 'action_masks': True},
                  gamma=0.995, learning_rate=1e-4, lr_schedule=None, kl_threshold=0.05, grad_norm=0.5, entropy_coef=0.005,
                  clip_value=False, critic_coef=1, value_bootstrap=False, use_action_masks=True, seq_length=8)
    cfg.pop('bounds_loss_coef')
    cfg.pop('bound_loss_type')
    cfg.update(over)
    return {'algo': {'name': 'a2c_discrete'}, 'model': {'name': 'multi_discrete_a2c' if multi else 'discrete_a2c'},
            'network': net, 'config': cfg}


def smac_rnn_cv_discrete(num_actors=8, agents=5, cell='lstm', units=128, layer_norm=False, state_dim=98, **over):
    """smac_rnn_discrete with the recurrent central value critic of the reference's `*_rnn_cv` SMAC runs
    (rl_games/configs/smac/v1/5m_vs_6m_rnn_cv.yaml, 3s_vs_5z_cv_rnn.yaml, 3m_torch_cv_rnn.yaml, runs/6h_vs_8z_rnn.yaml):
    `agents` agents per env, and over the env's privileged state (`state_dim`) a ReLU trunk [512, 256], one LSTM / GRU
    layer of `units` (optionally layer-normed) and one value column.  The critic's hyper-parameters follow
    5m_vs_6m_rnn_cv.yaml; its minibatch is half of the env-steps of a rollout."""
    cv_over = over.pop('central_value_config', {})
    params = smac_rnn_discrete(num_actors, cell=cell, units=units, layer_norm=layer_norm, **over)
    cfg = params['config']
    cfg['minibatch_size'] = over.get('minibatch_size', max(num_actors * agents * cfg['horizon_length'] // 2, 8))
    cfg['env_config'].update(state_dim=int(state_dim), agents=int(agents))
    cfg['central_value_config'] = {
        'minibatch_size': max(num_actors * cfg['horizon_length'] // 2, 8), 'mini_epochs': 4, 'learning_rate': 5e-4,
        'clip_value': False, 'normalize_input': True, 'truncate_grads': True, 'grad_norm': 2,
        'network': {'name': 'actor_critic', 'central_value': True,
                    'mlp': {'units': [512, 256], 'activation': 'relu', 'initializer': {'name': 'default'}},
                    'rnn': {'name': cell, 'units': units, 'layers': 1, 'layer_norm': bool(layer_norm)}}}
    cfg['central_value_config'].update(cv_over)
    return params


def clone(params):
    return copy.deepcopy(params)
