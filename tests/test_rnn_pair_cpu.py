"""CPU: what the four paired sequence entry points answer to malformed calls.

rlg_lstm_seq_forward_pair / _backward_pair and rlg_gru_seq_forward_pair / _backward_pair take the argument set of
their single entry twice (problem A, problem B) and one shape.  They check everything on the host and answer
hipErrorInvalidValue before they ask the HIP runtime for anything: an unsupported width, S or T <= 0, a NULL required
pointer in either problem, a w_hh of either problem that breaks the 128-unit forms' 16-byte rule, an output buffer of
A that is also the same-named buffer of B.  The pointers are small fake aligned addresses - the host code
dereferences none of them.

The table runs in a child process that sees no GPU, as tests/test_chain_entry_errors_cpu.py does: should a row ever
get past validation, its launch fails there, with the runtime's own code, instead of handing fake addresses to a
device.  One well-formed call per entry shows that code: it is not hipErrorInvalidValue, so a row that answers
hipErrorInvalidValue was stopped by the checks.

rlg_lstm_seq_backward_pair has no alignment row: launch_lstm_bwd_wide does not check w_hh (csrc/rnn_seq.hpp's list
of asymmetries) and the paired form inherits that.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = 1

# argument names of ONE problem, in ABI order; '?' marks the optional ones, '>' the buffers the kernel writes
_PROBLEM = {
    'rlg_lstm_seq_forward_pair': '>gates w_hh h0 c0 ?dones >out ?>c_all ?>hprev ?>h_final ?>c_final',
    'rlg_lstm_seq_backward_pair': 'gates c_all c0 ?dones w_hh d_out >d_gates',
    'rlg_gru_seq_forward_pair': '>gates w_hh b_hh h0 ?dones >out ?>hn_all ?>hprev ?>h_final',
    'rlg_gru_seq_backward_pair': 'gates hn_all hprev ?dones w_hh d_out >d_gx >d_gh',
}
_ALIGNED_W_HH = ('rlg_lstm_seq_forward_pair', 'rlg_gru_seq_forward_pair', 'rlg_gru_seq_backward_pair')


def _names(entry):
    return [n.lstrip('?>') for n in _PROBLEM[entry].split()]


def _required(entry):
    return [n.lstrip('>') for n in _PROBLEM[entry].split() if not n.startswith('?')]


def _outputs(entry):
    return [n.lstrip('?>') for n in _PROBLEM[entry].split() if '>' in n]


def _problem(entry, which):
    """a well-formed problem: every pointer given, 16-byte aligned, none shared with the other problem"""
    return {n: 0x100000 * (1 + 32 * which + k) for k, n in enumerate(_names(entry))}


def _rows():
    """(id, entry, A overrides, B overrides, shape overrides, rejected)"""
    t = []
    for e in _PROBLEM:
        def row(name, a=None, b=None, rejected=True, **shape):
            t.append((f'{e}: {name}', e, a or {}, b or {}, shape, rejected))

        row('well formed (reaches the runtime)', rejected=False)
        for h in (0, 12, 24, 48, 96, 256):
            row(f'width {h}', hidden=h)
        row('S = 0', num_seqs=0)
        row('S < 0', num_seqs=-3)
        row('T = 0', seq_len=0)
        row('T < 0', seq_len=-1)
        for n in _required(e):
            row(f'A without {n}', a={n: None})
            row(f'B without {n}', b={n: None})
            row(f'A without {n} at 128 units', a={n: None}, hidden=128)
        for n in _outputs(e):
            row(f'both problems write one {n}', b={n: _problem(e, 0)[n]})
            row(f'both problems write one {n} at 128 units', b={n: _problem(e, 0)[n]}, hidden=128)
        if e in _ALIGNED_W_HH:
            row('A: w_hh 4 bytes off at 128 units', a={'w_hh': _problem(e, 0)['w_hh'] + 4}, hidden=128)
            row('B: w_hh 8 bytes off at 128 units', b={'w_hh': _problem(e, 1)['w_hh'] + 8}, hidden=128)
    return t


def run_table():
    """{row id: code} of the library that rl_games_amd._lib selects"""
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, entry, a_over, b_over, shape, _ in _rows():
        assert name not in codes, name
        a, b = dict(_problem(entry, 0), **a_over), dict(_problem(entry, 1), **b_over)
        dims = dict(dict(num_seqs=5, seq_len=4, hidden=64), **shape)
        args = [a[n] for n in _names(entry)] + [b[n] for n in _names(entry)]
        codes[name] = getattr(lib, entry)(*args, dims['num_seqs'], dims['seq_len'], dims['hidden'], None)
    return codes


def test_malformed_paired_calls_are_rejected_on_the_host():
    env = dict(os.environ)
    # no device for the child: a row that validation let through by mistake must not reach one
    env['HIP_VISIBLE_DEVICES'] = '-1'
    env['CUDA_VISIBLE_DEVICES'] = '-1'
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    rows = _rows()
    assert len(rows) >= 140
    assert set(codes) == {r[0] for r in rows}
    wrong = {name: codes[name] for name, *_, rejected in rows if (codes[name] == INVALID) != rejected}
    assert not wrong, f'codes of the rows that were (not) rejected against the table: {wrong}'
    # the well-formed calls came back from a runtime without a device: an error, but its own
    assert all(codes[name] != 0 for name, *_, rejected in rows if not rejected)


def test_the_pair_keeps_two_launches_for_the_one_slower_shape_class():
    """chain_net.paired_launch_pays: profiles/separate_rnn.txt's rule - the 128-unit LSTM forward at T = 1 with more
    paired workgroups than CUs - and nothing else."""
    from rl_games_amd.chain_net import paired_launch_pays
    assert not paired_launch_pays('lstm', 128, 'forward', 4096, 1)
    assert not paired_launch_pays('lstm', 128, 'forward', 2049, 1)
    assert paired_launch_pays('lstm', 128, 'forward', 2048, 1)
    for cell, hidden, direction, S, T in (('lstm', 128, 'backward', 4096, 1), ('lstm', 128, 'forward', 4096, 16),
                                          ('gru', 128, 'forward', 4096, 1), ('lstm', 64, 'forward', 4096, 1),
                                          ('lstm', 128, 'forward', 24, 1)):
        assert paired_launch_pays(cell, hidden, direction, S, T), (cell, hidden, direction, S, T)


if __name__ == '__main__':
    print(json.dumps(run_table()))
