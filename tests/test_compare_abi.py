"""CPU tests of what only libstackrl_compare.so has at its boundary: the size of a record, held to the host's own count.  The
boundary it shares with the other libraries is held in tests/test_abi.py, tests/test_build_deps.py and tests/test_isa_guard.py."""


def test_record_doubles_is_the_hosts_count():
  from stackrl_amd import compare
  lib = compare.load()
  for P in range(0, 10):
    assert lib.srl_compare_record_doubles(P) == (compare.record_doubles(P) if 1 <= P <= 8 else 0)
  assert compare.record_doubles(8) == 189 and compare.MAX_POLICIES == 8
