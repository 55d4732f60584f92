"""bench.py with DSA_ALGO_FULL_CHAINS forced on every tuned mel-cepstral forward launch (same arguments as bench.py): the A/B partner
of the coarse Newton steps -- its --dump-outputs must be byte-identical to the dump of the kernels before them, and its timing
prices the step loop's extra control flow."""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsptk_amd.ops import mcep as _m
_m._full_chains[0] = True
sys.argv[0] = os.path.join(ROOT, "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")
