"""Borrowing the library's process-wide tuning knobs (migan_set_tuning) for a test.  Test infrastructure only.

The knobs live in the loaded library, so whatever a test leaves behind plans every later test of the process.  Nothing
here knows a default: a knob goes back to the value it had, which may be what a MIGAN_* variable chose for the run."""
import contextlib


@contextlib.contextmanager
def knobs(lib, **values):
    """set the given knobs for the body, then put back what was there (also when the body raises)"""
    before = {key: lib.get_tuning(key) for key in values}
    try:
        for key, value in values.items():
            lib.set_tuning(key, value)
        yield
    finally:
        for key, value in before.items():
            lib.set_tuning(key, value)
