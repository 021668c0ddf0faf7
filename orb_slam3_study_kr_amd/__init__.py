"""MI355X-native local bundle adjustment + ORB Hamming matching (ORB-SLAM3 hot path).

Product code: ``csrc/`` (HIP kernels + C-ABI, built into ``csrc/liborbslam3_hip.so``),
``csrc/host/`` (the C++ drop-in sources an integrator compiles into their ORB-SLAM3 tree),
``capi`` (ctypes mirror of include/orbslam3_hip.h), ``lba`` / ``orb`` (thin Python
drivers over the C-ABI), ``synth`` (synthetic inputs).  Test only: ``csrc/hosttest/``
(stand-in class bodies and the C wrappers of include/orbslam3_hip_host.h), built with
``csrc/host/`` into ``csrc/liborbslam3_hip_hosttest.so`` and driven by ``host``.  The CPU
oracle lives in ``/oracle`` and is never imported from this package.
"""
__version__ = "0.1.0"
