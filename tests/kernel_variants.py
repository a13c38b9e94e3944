"""Kernel-variant bits by name (rt_api.h rt_debug_set_variant; csrc/rt_internal.h VariantBit), shared by the
GPU parity and edge tests, tests/variants_check.py and the CPU test of the dispatch plan."""

# variant bits the product library serves itself (rt_api.h rt_debug_set_variant)
VARIANTS = {"xcd-order": 4, "xcd-runs-4": 512, "dispatch-order": 1536, "full-8-waves": 8192, "full-small-build": 16384,
            "split-primary": 32768, "generic-depth-kernel": 65536, "coarse-cost-buckets": 262144,
            "primary-binary-tree": 2097152}
# the A/B kernels of the variants library only (rt_variants.hip, `make variants`)
VARIANTS_LIB = {"vgpr-stack": 1, "wide4": 2, "full-pipeline": 16, "pipeline-lane-refl": 48,
                "pipeline-lane-all": 16 | 32 | 64 | 128, "two-rays-per-lane": 256, "persistent": 2048,
                "persistent-no-steal": 2048 | 4096, "dual-chain": 1048576}
# longest-first dispatch knobs of the product library: never / also with frames in flight (A/B only)
NO_LPT, LPT_IN_FLIGHT = 131072, 524288
