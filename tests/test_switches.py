"""The TMJX_* environment variables the package reads are exactly those DESIGN.md's table of switches lists (source text only: no library, no GPU)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
READ = re.compile(r'(?:\benviron(?:\.get)?|\bgetenv|\benv\.get)\s*[(\[]\s*"(TMJX_[A-Z0-9_]+)"')
ROW = re.compile(r"^\| `(TMJX_[A-Z0-9_]+)` \|", re.M)


def test_every_environment_switch_the_package_reads_is_in_the_design_table():
    read = set()
    for path in (ROOT / "track_mjx_amd").rglob("*"):
        if path.suffix in (".py", ".hip", ".h") and ".build" not in path.parts:
            read |= set(READ.findall(path.read_text()))
    listed = set(ROW.findall((ROOT / "DESIGN.md").read_text()))
    assert len(read) >= 10, "the scan found almost nothing: the pattern no longer matches how the code reads its environment"
    assert read == listed, f"read but not in DESIGN.md's table: {sorted(read - listed)}; listed but no longer read: {sorted(listed - read)}"
