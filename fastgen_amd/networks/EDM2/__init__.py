from fastgen_amd.networks.EDM2.network import EDM2Precond  # noqa: F401
