"""Device memory has one owner type in the C library (mer::DeviceBuffer and its pinned-host twin, mitsubaer_amd/csrc/mer_internal.hpp): no other
source file allocates or frees device or pinned memory, and the flag that once said whether a volume owned its dense data is gone."""
import glob
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mitsubaer_amd", "csrc")
OWNER = "mer_internal.hpp"
CALLS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) > 20 and os.path.join(CSRC, OWNER) in files
    return {os.path.basename(f): open(f).read() for f in files}


def test_only_the_owner_type_allocates_and_frees():
    src = _sources()
    for call in CALLS:
        assert call in src[OWNER], call
    # hipMallocAsync( and the like do not contain these spellings; a match is the call itself, wherever it stands (comments included)
    found = sorted((name, call) for name, text in src.items() if name != OWNER for call in CALLS if call in text)
    assert found == []


def test_owns_dense_is_gone():
    assert [name for name, text in _sources().items() if "owns_dense" in text] == []
