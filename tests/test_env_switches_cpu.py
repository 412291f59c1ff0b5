"""The table of environment switches in DESIGN.md (section 9) against the source: the RC_* names that csrc/ passes to env_int or getenv
are exactly the names in the table's first column, each read where the table says, and nothing but env_int calls getenv."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rusty_compression_amd", "csrc")
READ = re.compile(r'\b(env_int|getenv)\s*\(\s*"(RC_[A-Z0-9_]+)"')


def switches_in_source():
    """{name: {file, ...}} of every RC_* name read from the environment under csrc/."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            for _, switch in READ.findall(open(os.path.join(CSRC, name)).read()):
                found.setdefault(switch, set()).add(name)
    return found


def switches_in_table():
    """{name: the row's file column} of the table whose header row begins with | switch | default | file |."""
    lines = open(os.path.join(ROOT, "DESIGN.md")).read().split("\n")
    start = next(i for i, line in enumerate(lines) if line.startswith("| switch | default | file |"))
    table = {}
    for line in lines[start + 2:]:
        if not line.startswith("|"):
            break
        cells = [c.strip() for c in re.split(r"(?<!\\)\|", line)[1:-1]]
        assert len(cells) == 5, line
        m = re.fullmatch(r"`(RC_[A-Z0-9_]+)`", cells[0])
        assert m, f"first column is not one switch: {cells[0]}"
        assert m.group(1) not in table, f"{m.group(1)} is listed twice"
        assert cells[1] and cells[3] and cells[4], line
        table[m.group(1)] = cells[2]
    return table


def test_the_table_lists_exactly_the_switches_the_source_reads():
    src, table = switches_in_source(), switches_in_table()
    assert len(src) >= 20  # the pattern still finds the reads
    assert set(table) == set(src), (sorted(set(src) - set(table)), sorted(set(table) - set(src)))


def test_every_switch_is_read_in_the_file_the_table_names():
    table = switches_in_table()
    for switch, files in switches_in_source().items():
        for f in files:
            assert f"`{f}`" in table[switch], f"{switch} is read in {f}, the table says {table[switch]}"


def test_getenv_is_called_by_env_int_alone_and_each_switch_is_read_at_one_site():
    calls = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
                code = line.split("//")[0]
                if re.search(r"\bgetenv\s*\(", code):
                    calls.append((name, i))
    assert len(calls) == 1 and calls[0][0] == "rc_common.hpp", calls
    text = "".join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".hpp")))
    reads = [s for _, s in READ.findall(text)]
    # the GEMM's two split-K planners each read the two targets they share; every other switch has one site
    twice = {"RC_GEMM_TARGET_WGS", "RC_GEMM_SMALL_TARGET"}
    for s in set(reads):
        assert reads.count(s) == (2 if s in twice else 1), (s, reads.count(s))
