#!/usr/bin/env python3
"""Layout dump of the UNet plan, on the CPU: creates (and destroys) a plan for every configuration of a fixed grid and
writes, per configuration, drs_unet_packed_bytes / workspace_bytes / packed_bwd_bytes and a hash over every (parameter name,
numel) and (tensor name, n, c, h, w).  Two builds of the library lay their plans out alike iff their dumps are equal:
run it once per build (DRS_LIB selects the library) under the same kernel-family switches (DRS_SP, DRS_FL, DRS_UPFUSE, ...)
and compare the files, or the digest it prints.  No GPU is needed: plan creation makes no HIP call.
Usage: plan_dump.py OUT.json"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionremotesensing_amd import _lib  # noqa: E402

# (name, variant, magnification, conditioning channels (None: the image's), classes)
VARIANTS = [("superres_x2", _lib.VARIANT_SUPERRES, 2, None, 0), ("superres_x4", _lib.VARIANT_SUPERRES, 4, None, 0),
            ("sar_to_ndvi", _lib.VARIANT_SAR_TO_NDVI, 1, 2, 0), ("generation_10", _lib.VARIANT_GENERATION, 1, 0, 10),
            ("generation_0", _lib.VARIANT_GENERATION, 1, 0, 0)]
IMPLS = [_lib.IMPL_DIRECT, _lib.IMPL_MFMA_F32, _lib.IMPL_MFMA_BF16X3, _lib.IMPL_MFMA_F16]
FLAGS = [0, _lib.PLAN_KEEP_ALL, _lib.PLAN_TRAIN]
SIZES = [32, 64, 128, 256]
BANDS = [1, 3, 16]
BATCHES = [1, 2, 16]


def dump_one(lib, name, variant, mag, cond, classes, impl, flags, size, bands, batch):
    cfg = _lib.UNetConfig(batch, batch, bands, bands, size, size, mag, impl, 1e-5, flags, variant,
                          bands if cond is None else cond, classes)
    plan = C.c_void_p()
    _lib.check(lib.drs_unet_plan_create(C.byref(plan), C.byref(cfg)), "drs_unet_plan_create")
    try:
        h = hashlib.sha256()
        for i in range(lib.drs_unet_num_params(plan)):
            h.update(b"%s %d\n" % (lib.drs_unet_param_name(plan, i), lib.drs_unet_param_numel(plan, i)))
        shape = [C.c_int() for _ in range(4)]
        for i in range(lib.drs_unet_num_tensors(plan)):
            _lib.check(lib.drs_unet_tensor_shape(plan, i, *[C.byref(v) for v in shape]), "drs_unet_tensor_shape")
            h.update(b"%s %d %d %d %d\n" % ((lib.drs_unet_tensor_name(plan, i),) + tuple(v.value for v in shape)))
        return {"variant": name, "impl": impl, "flags": flags, "size": size, "bands": bands, "batch": batch,
                "packed_bytes": lib.drs_unet_packed_bytes(plan), "workspace_bytes": lib.drs_unet_workspace_bytes(plan),
                "packed_bwd_bytes": lib.drs_unet_packed_bwd_bytes(plan), "names_and_shapes": h.hexdigest()}
    finally:
        lib.drs_unet_plan_destroy(plan)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    lib = _lib.load()
    rows = [dump_one(lib, *v, impl, flags, size, bands, batch)
            for v, impl, flags, size, bands, batch in itertools.product(VARIANTS, IMPLS, FLAGS, SIZES, BANDS, BATCHES)]
    text = json.dumps({"abi_version": lib.drs_abi_version(), "plans": rows}, indent=0) + "\n"
    with open(sys.argv[1], "w") as f:
        f.write(text)
    print(f"{len(rows)} plans, sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
