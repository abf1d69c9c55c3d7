"""Static guard of the third-generation walk's LDS traffic (enum_walk_kernel<MU_LDS, DUAL, CHAIN = true>, DESIGN.md
section 3): the LDS unit is shared by the four SIMDs of a CU and every ds_bpermute_b32 per node costs node time, so
the first child's distance is computed by every lane from wave-uniform operands (nd + a1 * a1 * r) instead of being
broadcast from lane 0 of the 64-lane test.

In the EXPAND loop of all four CHAIN = true instantiations: the chain-descent block (the block that counts the child
without a writelane) holds no ds_ instruction at all, and the whole loop holds at most two ds_bpermute_b32 (the two
halves of the centre) and one ds_write (the column push of the descent with siblings); the MU_LDS instantiations also
read the mu row from LDS, which is no crossbar traffic of the walk itself.

CPU-only: built on the helpers of test_isa_walk.py (hipcc emits the ISA for gfx950 once for the module)."""
import pytest

from test_isa_walk import KERNEL, _blocks, _expand_loop, _kernel_body, artefacts, pytestmark  # noqa: F401


@pytest.mark.parametrize("mu_lds,dual", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_walk3_expand_loop_broadcasts_the_centre_only(artefacts, mu_lds, dual):
    _, asm = artefacts
    loop = _expand_loop(_kernel_body(asm, KERNEL % (mu_lds, dual, 1)))
    assert loop is not None
    adds = [b for b in loop if any(s.startswith("v_addc_co_u32") for s in b[2])]
    chain = [b for b in adds if not any(s.startswith("v_writelane") for s in b[2])]
    assert len(chain) == 1, [b[0] for b in adds]
    ds_chain = [s for s in chain[0][2] if s.startswith("ds_")]
    assert not ds_chain, ds_chain
    ins = [s for b in loop for s in b[2]]
    ds = [s for s in ins if s.startswith("ds_")]
    bperm = [s for s in ds if s.startswith("ds_bpermute_b32")]
    writes = [s for s in ds if s.startswith("ds_write")]
    other = [s for s in ds if s not in bperm and s not in writes]
    assert len(bperm) <= 2 and len(writes) <= 1, ds
    # (nothing else goes through the LDS unit but the mu row of the MU_LDS instantiations)
    assert all(s.startswith("ds_read_b64") for s in other) and len(other) <= (1 if mu_lds else 0), ds
