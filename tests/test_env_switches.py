"""Every environment switch the library reads is documented, and every
documented one exists: the getenv("MGIC_...") names of csrc against the
"Kernel switches" paragraph of INTEGRATION.md."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# runtime settings of the IPC transport: INTEGRATION.md describes them with
# the transport, not in the "Kernel switches" paragraph
IPC_SETTINGS = {
    "MGIC_IPC_ARENA_MB",
    "MGIC_IPC_TIMEOUT_S",
    "MGIC_IPC_BLOCK_ELEMS",
    "MGIC_IPC_GRID_CAP",
}


def _read_by_the_library():
    names = set()
    for ext in ("hip", "cpp", "hpp"):
        for path in glob.glob(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "*." + ext)):
            with open(path) as f:
                names.update(re.findall(r'getenv\(\s*"(MGIC_[A-Z0-9_]+)"', f.read()))
    return names


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    missing = sorted(n for n in IPC_SETTINGS if n not in text)
    assert not missing, f"IPC settings INTEGRATION.md does not describe: {missing}"
    start = text.index("* **Kernel switches.**")
    end = text.index("\n* **", start + 1)  # the next bullet
    return set(re.findall(r"MGIC_[A-Z0-9_]+", text[start:end]))


def test_env_switches_match_the_documented_ones():
    code, doc = _read_by_the_library(), _documented()
    assert code, "no getenv(\"MGIC_...\") found: the scan is broken"
    assert IPC_SETTINGS <= code, sorted(IPC_SETTINGS - code)
    assert not (doc & IPC_SETTINGS), "IPC settings moved into the paragraph: drop them from IPC_SETTINGS"
    undocumented = code - IPC_SETTINGS - doc
    stale = doc - code
    assert not undocumented, f"read by csrc, missing from INTEGRATION.md: {sorted(undocumented)}"
    assert not stale, f"in INTEGRATION.md, read by nothing in csrc: {sorted(stale)}"

