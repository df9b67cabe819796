"""No GPU needed: the host state of the library that include/lgteun_hip.h calls thread-local -- the message behind lg_last_error (g_err,
csrc/common.h) -- under eight concurrent host threads, and the workspace sizers called from all of them at once.

The calls are those of tests/test_abi_limits_cpu.py: ONE argument outside its range, pointers that are never dereferenced (limits_helpers.FAKE),
a validator that rejects the call before any HIP call.  ctypes releases the GIL inside the library, so the eight threads really are inside it
together; a barrier in front of every call makes the eight calls start as close to each other as the host allows, and a second barrier between
a call and the read of its message lets every other thread's call finish first -- a message kept in one process-wide buffer would then be the
LAST thread's for all eight."""
import threading

from lgteun_amd import _lib
from test_abi_limits_cpu import ENTRIES, HIP_WORDS, all_sizers, SIZER_NAMES, BS

N_THREADS = 8
ROUNDS = 50           # host-only calls of a few microseconds: 50 rounds of 8 calls take milliseconds

# one rejection per thread, every one another entry AND another argument: (entry, the bad argument, what the message must say)
PER_THREAD = [
    ('lg_sfim', dict(B=0), 'B must be'),
    ('lg_gsa', dict(stats=ENTRIES['lg_gsa'][2]['stats'] + 4), 'stats must be 8-byte aligned'),
    ('lg_mtf_glp', dict(n_taps=65), 'n_taps must be'),
    ('lg_bdsd', dict(block=48), 'block must be'),
    ('lg_iqa_ref', dict(C=17), 'C must be'),
    ('lg_qnr_grad', dict(B_global=1), 'B_global must be at least B'),
    ('lg_scene_blend', dict(overlap=12), 'overlap'),
    ('lg_fir_decimate4', dict(phase=4), 'phase'),
]


def _reject(entry, bad):
    prefix, names, good = ENTRIES[entry]
    names = names.split()
    args = dict(good, stream=None)
    args.update(bad)
    return getattr(_lib.lib(), entry)(*[args[n] for n in names])


def _run_threads(target):
    """start N_THREADS threads on target(i), join them, re-raise the first failure"""
    errors = [None] * N_THREADS

    def body(i):
        try:
            target(i)
        except BaseException as e:          # noqa: BLE001 - a failed assertion in a thread must fail the test
            errors[i] = e
    threads = [threading.Thread(target=body, args=(i,)) for i in range(N_THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
        assert not t.is_alive(), 'a thread did not come back'
    for e in errors:
        if e is not None:
            raise e


def test_the_eight_rejections_are_eight_different_messages_on_one_thread():
    """the condition of the next test: single-threaded, every case is rejected with its own message, so a mix-up would show"""
    assert len(PER_THREAD) == N_THREADS and len({e for e, _, _ in PER_THREAD}) == N_THREADS
    assert len({next(iter(b)) for _, b, _ in PER_THREAD}) == N_THREADS
    msgs = []
    for entry, bad, says in PER_THREAD:
        rc = _reject(entry, bad)
        msg = _lib.lib().lg_last_error().decode()
        assert rc < 0 and msg.startswith(ENTRIES[entry][0] + ':') and says in msg, (entry, bad, rc, msg)
        assert not any(w in msg.lower() for w in HIP_WORDS), msg
        msgs.append(msg)
    assert len(set(msgs)) == N_THREADS
    for i, (entry, _, _) in enumerate(PER_THREAD):          # no message passes another thread's check
        assert [j for j, m in enumerate(msgs) if m.startswith(ENTRIES[entry][0] + ':')] == [i], (entry, msgs)


def test_lg_last_error_is_per_thread():
    barrier = threading.Barrier(N_THREADS)
    L = _lib.lib()

    def work(i):
        entry, bad, says = PER_THREAD[i]
        prefix = ENTRIES[entry][0] + ':'
        for r in range(ROUNDS):
            barrier.wait(30)
            rc = _reject(entry, bad)
            barrier.wait(30)                     # every thread's call has returned: a shared buffer now holds someone else's message
            msg = L.lg_last_error().decode()
            assert rc < 0, (i, r, entry, rc)
            assert msg.startswith(prefix) and says in msg, (i, r, entry, 'read the message of another thread', msg)
    _run_threads(work)


def test_a_thread_that_made_no_call_reads_no_other_threads_message():
    """a fresh thread's message is its own (empty) one, whatever the main thread was told last"""
    rc = _reject(*PER_THREAD[0][:2])
    mine = _lib.lib().lg_last_error().decode()
    assert rc < 0 and mine
    seen = []
    t = threading.Thread(target=lambda: seen.append(_lib.lib().lg_last_error().decode()))
    t.start()
    t.join(30)
    assert seen == [''], seen
    assert _lib.lib().lg_last_error().decode() == mine


def test_sizers_return_the_single_thread_values_from_eight_threads():
    """every sizer of test_abi_limits_cpu at the largest accepted shape over its ladder of B, and over the sides at B = 65535, from eight threads
    at once: the values of one thread alone"""
    sizers = all_sizers()
    alone = {name: ([sizers[name][0](B) for B in BS], sizers[name][1]()) for name in SIZER_NAMES}
    assert all(v[0][0] > 0 for v in alone.values())
    barrier = threading.Barrier(N_THREADS)

    def work(i):
        order = SIZER_NAMES[i:] + SIZER_NAMES[:i]          # every thread starts at another sizer
        for r in range(3):
            barrier.wait(30)
            for name in order:
                got = ([sizers[name][0](B) for B in BS], sizers[name][1]())
                assert got == alone[name], (i, r, name)
    _run_threads(work)
