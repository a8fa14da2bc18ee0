"""CPU: libwekws_hip_hooks.so runs the product's own kernels.

The test library (make hooks) links the very objects of libwekws_hip.so but one: wekws_hip_hooks.hip, compiled with -DWEKWS_TEST_HOOKS.  So
every GPU suite that loads it -- the route, fbank and softmax matrices, the GRU epoch and tenant tests, the forward_streams matrix --
holds to the oracle the code objects that tests/test_isa_hazard.py scans, not a second compilation of them.  Checked on what was built:
the gfx950 code objects of the two libraries are the same bytes, except for that one unit's, which holds no kernel in the product
library (so the product library has no code object for it, or one without a kernel) and exactly debug_hog_kernel in the test library."""
import os
import struct

import pytest

from tests.test_isa_hazard import LIB, OBJDUMP, code_objects

HOOKS = os.path.join(os.path.dirname(LIB), "libwekws_hip_hooks.so")


def kernels(elf):
    """Names of the kernels an AMDGPU code object defines: a kernel `k` comes with its descriptor, the symbol `k.kd`."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, off, size, link, _, _, entsize in sections:
        if kind not in (2, 11):                                # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for at in range(off, off + size, entsize):
            name_at, _, _, shndx = struct.unpack_from("<IBBH", elf, at)
            name = elf[stroff + name_at:elf.index(b"\0", stroff + name_at)].decode()
            if shndx and name.endswith(".kd"):
                names.add(name[:-3])
    return names


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="library not built or llvm-objdump missing")
def test_the_test_library_shares_every_kernel_object_with_the_product_library():
    assert os.path.exists(HOOKS), "make hooks builds libwekws_hip_hooks.so next to libwekws_hip.so"
    product = list(code_objects(open(LIB, "rb").read()))
    hooks = list(code_objects(open(HOOKS, "rb").read()))
    assert len(product) >= 10 and len(product) == len(set(product)) and len(hooks) == len(set(hooks))
    only_product = [co for co in product if co not in set(hooks)]
    only_hooks = [co for co in hooks if co not in set(product)]
    # the product's own build of that unit holds no kernel: the compiler then embeds no code object for it at all (or an empty one)
    assert len(only_product) <= 1 and len(only_hooks) == 1, (len(only_product), len(only_hooks))
    assert all(kernels(co) == set() for co in only_product)
    assert kernels(only_hooks[0]) == {"debug_hog_kernel"}
    assert sum(len(kernels(co)) for co in product) >= 50      # (the parser does see kernels where there are some)
