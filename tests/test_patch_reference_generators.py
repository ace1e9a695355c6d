"""patch.install(generator_rng=...) on the REAL reference modules (oracle/_ref, where build() found a checkout of the
reference): the checks of tests/generators_harness.py that tests/test_generators_host.py runs on the stand-in package.  In
a file of its own behind tests/test_patch_reference.py, which loads the reference once for the process."""

from __future__ import annotations

import pytest

import generators_harness as gh

NO_REF = "the reference modules are not in oracle/_ref (build() copies them where a checkout of the reference exists)"


@pytest.fixture(scope="module")
def ref():
    package = gh.reference_package()
    if package is None:
        pytest.skip(NO_REF)
    return package


def test_patched_generator_step_is_a_drop_in_on_the_reference(ref):
    gh.check_patched_generator_step_is_a_drop_in(*ref)


def test_the_rebound_method_keeps_the_references_signature_and_return_type(ref):
    gh.check_the_rebound_method_keeps_the_references_signature_and_return_type(*ref)


def test_install_without_generator_rng_leaves_the_method_alone_on_the_reference(ref):
    gh.check_install_without_generator_rng_leaves_the_method_alone(*ref)
