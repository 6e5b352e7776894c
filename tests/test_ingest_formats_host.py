"""No GPU: pins the Python restatement of the FASTA / one-read-per-line rules (ingest_formats_common.py), against which
test_ingest_formats.py checks the device's record scan, to `gram`'s general host reader — the `slow` line of `gram _parse_check`
(reads, bases, FNV-1a of offsets and bases) on every generated file of that test."""
import pytest

from ingest_formats_common import generated_files, gram, parse, parse_check_line, parse_check_lines

FILES = generated_files()


@pytest.mark.parametrize("name,kind,data", FILES, ids=[f[0] for f in FILES])
def test_restatement_equals_the_host_reader(tmp_path, name, kind, data):
    path = tmp_path / (name + (".fa" if kind == "fasta" else ".txt"))
    path.write_bytes(data)
    out = gram("_parse_check", str(path), "2")
    assert out.returncode == 0, out.stdout
    lines = parse_check_lines(out)
    assert lines["fast"] == "declined", out.stdout
    assert lines["slow"] == parse_check_line(parse(kind, data)), out.stdout
