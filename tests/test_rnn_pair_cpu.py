"""CPU: what the four sequence entry points answer to malformed calls.

rlg_lstm_seq_forward / _backward and rlg_gru_seq_forward / _backward take an array of one or two problem descriptors
and one shape.  They check everything on the host and answer hipErrorInvalidValue before they ask the HIP runtime for
anything: a NULL array or a count other than 1 or 2, an unsupported width, S or T <= 0, a NULL required pointer in any
problem, a w_hh of any problem that breaks the 128-unit forms' 16-byte rule and, with two problems, an output buffer
of A that is also the same-named buffer of B.  The pointers are small fake aligned addresses - the host code
dereferences none of them.

The table runs in a child process that sees no GPU, as tests/test_chain_entry_errors_cpu.py does: should a row ever
get past validation, its launch fails there, with the runtime's own code, instead of handing fake addresses to a
device.  One well-formed call per entry and count shows that code: it is not hipErrorInvalidValue, so a row that
answers hipErrorInvalidValue was stopped by the checks.

rlg_lstm_seq_backward has no alignment rule: launch_lstm_bwd_wide does not check w_hh (csrc/rnn_seq.hpp's list of
asymmetries), with one problem or two; its off-alignment rows are "not rejected".

The fields' positions come from the ctypes mirrors of the descriptors (rl_games_amd/_lib.py); which of them are
required and which are written is stated here, by name, so a mirror whose order is not the header's fails the rows of
the fields it misplaces.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = 1

# entry: (descriptor class of _lib, the optional fields, the buffers the kernel writes)
_ENTRIES = {
    'rlg_lstm_seq_forward': ('LstmFwd', 'dones c_all hprev hT cT', 'gates out c_all hprev hT cT'),
    'rlg_lstm_seq_backward': ('LstmBwd', 'dones', 'd_gates'),
    'rlg_gru_seq_forward': ('GruFwd', 'dones hn_all hprev hT', 'gates out hn_all hprev hT'),
    'rlg_gru_seq_backward': ('GruBwd', 'dones', 'd_gx d_gh'),
}
_ALIGNED_W_HH = ('rlg_lstm_seq_forward', 'rlg_gru_seq_forward', 'rlg_gru_seq_backward')


def _descriptor(entry):
    from rl_games_amd import _lib
    return getattr(_lib, _ENTRIES[entry][0])


def _names(entry):
    return [n for n, _ in _descriptor(entry)._fields_]


def _required(entry):
    return [n for n in _names(entry) if n not in _ENTRIES[entry][1].split()]


def _outputs(entry):
    return [n for n in _names(entry) if n in _ENTRIES[entry][2].split()]


def _problem(entry, which):
    """a well-formed problem: every pointer given, 16-byte aligned, none shared with the other problem"""
    return {n: 0x100000 * (1 + 32 * which + k) for k, n in enumerate(_names(entry))}


def _rows():
    """(id, entry, num_problems, A overrides, B overrides, shape overrides, rejected); the shape override
    `no_array` passes NULL for the descriptor array"""
    t = []
    for e in _ENTRIES:
        def row(name, count=2, a=None, b=None, rejected=True, **shape):
            t.append((f'{e}: {name}', e, count, a or {}, b or {}, shape, rejected))

        # two problems
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

        # one problem
        row('single: well formed (reaches the runtime)', 1, rejected=False)
        for h in (0, 12, 24, 48, 96, 256):
            row(f'single: width {h}', 1, hidden=h)
        row('single: S = 0', 1, num_seqs=0)
        row('single: S < 0', 1, num_seqs=-3)
        row('single: T = 0', 1, seq_len=0)
        row('single: T < 0', 1, seq_len=-1)
        for n in _required(e):
            row(f'single: without {n}', 1, a={n: None})
            row(f'single: without {n} at 128 units', 1, a={n: None}, hidden=128)
        row('single: w_hh 4 bytes off at 128 units', 1, a={'w_hh': _problem(e, 0)['w_hh'] + 4}, hidden=128,
            rejected=e in _ALIGNED_W_HH)

        # the array itself
        row('no array', 1, no_array=True)
        row('0 problems', 0)
        row('3 problems', 3)
        row('-1 problems', -1)
    return t


def run_table():
    """{row id: code} of the library that rl_games_amd._lib selects"""
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, entry, count, a_over, b_over, shape, _ in _rows():
        assert name not in codes, name
        problems = (_descriptor(entry) * 2)()
        for desc, fields in zip(problems, (dict(_problem(entry, 0), **a_over), dict(_problem(entry, 1), **b_over))):
            for n, v in fields.items():
                setattr(desc, n, v)
        dims = dict(dict(num_seqs=5, seq_len=4, hidden=64, no_array=False), **shape)
        codes[name] = getattr(lib, entry)(None if dims['no_array'] else problems, count, dims['num_seqs'],
                                          dims['seq_len'], dims['hidden'], None)
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
    assert len(rows) >= 257
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
