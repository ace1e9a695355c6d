"""Recipe of oracle/_ref/ (TEST INFRASTRUCTURE — never imported by the product).

The drop-in tests (tests/test_patch_reference.py, tests/test_standin_drift.py) run the UNMODIFIED reference modules.
Their program text is not part of this repository: build() copies the reference package's modules from a checkout of
the reference into oracle/_ref/distributed_keygen/, which stays out of version control, and the tests import them from
there (with the dependency stand-ins of tests/golden/make_golden.py).  Where no checkout of the reference is at hand,
nothing is copied and those tests skip.

The checkout is found through MX_REFERENCE_SRC (its root directory), else at DEFAULT_SRC, where the build container
keeps it.
"""

from __future__ import annotations

import os
import shutil
from pathlib import Path

HERE = Path(__file__).resolve().parent
REF_DIR = HERE / "_ref"
REF_PKG = REF_DIR / "distributed_keygen"          # what the tests import
DEFAULT_SRC = Path("/root/reference")
PKG_IN_CHECKOUT = Path("src/tno/mpc/protocols/distributed_keygen")
MODULES = ("__init__.py", "distributed_keygen.py", "paillier_shared_key.py", "utils.py")


def source_package() -> Path:
    return Path(os.environ.get("MX_REFERENCE_SRC") or DEFAULT_SRC) / PKG_IN_CHECKOUT


def build(verbose: bool = False) -> Path | None:
    """Copy the reference's modules into oracle/_ref/distributed_keygen/ when a readable checkout exists; returns the
    package directory, or None when there is nothing to copy (an existing copy is then left as it is)."""
    src = source_package()
    try:
        if not all(os.access(src / m, os.R_OK) for m in MODULES):
            return None
        REF_PKG.mkdir(parents=True, exist_ok=True)
        for m in MODULES:
            if not (REF_PKG / m).exists() or (REF_PKG / m).read_bytes() != (src / m).read_bytes():
                shutil.copyfile(src / m, REF_PKG / m)
    except OSError as exc:
        if verbose:
            print(f"oracle/_ref: reference not copied ({exc})")
        return None
    if verbose:
        print(f"oracle/_ref: {len(MODULES)} reference modules in {REF_PKG}")
    return REF_PKG


if __name__ == "__main__":
    print(build(verbose=True))
