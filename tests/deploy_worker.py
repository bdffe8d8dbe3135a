"""One role of tests/test_gpu_deploy.py, run as a fresh interpreter: the command line of dctfhe.deploy (python -m dctfhe.deploy ...), then the
check that this process imported neither the compiler nor torch -- a client, a data owner and a server start from files alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dct-cryptonets_amd"))


def main():
    from dctfhe import deploy
    deploy.main(sys.argv[1:])
    loaded = [m for m in ("torch", "dctfhe.compile", "dctfhe.models", "dctfhe.torch_import", "dctfhe.quantized_module") if m in sys.modules]
    if loaded:
        print("role process imported", loaded)
        return 3
    print("ROLE OK", sys.argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
