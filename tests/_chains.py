"""Test support: the named chains of the suite -- fixture files and generated chains by name, as library chains, oracle chains or both.
Chains are identified by name and seed throughout the suite; nothing here touches a device."""
import os

from conftest import FIXTURES
from rosdyn_amd.urdf_gen import generated_long_chain, generated_revolute_chain


GRAV = (0.0, 0.0, -9.806)

PERMUTED_12 = ["j13", "j0", "j9", "j4", "j16", "j1", "j7", "j19", "j3", "j10", "j6", "j12"]

FILES = {
    "ur10_like": ("ur10_like.urdf", "base_link", "tool0"),
    "ur10_public": ("ur10_public.urdf", "base_link", "tool0"),
    "panda_like": ("panda_like.urdf", "link0", "hand"),
    "mixed_joints": ("mixed_joints.urdf", "world", "tip"),
    "ur10_public_long": ("ur10_public_long.urdf", "base_link", "tcp"),
    "planar_2r": ("planar_2r.urdf", "base", "l2"),
}
SWEPT = list(FILES) + ["rev%d" % k for k in range(1, 11)]
CHUNKED = ["rev14", "rev20", "rev32", "gen20", "gen32", "gen20_permuted"]
CHAINS = SWEPT + CHUNKED


def _spec(name):
    if name in FILES:
        f, base, tool = FILES[name]
        return os.path.join(FIXTURES, f), base, tool, None
    if name.startswith("rev"):
        nj = int(name[3:])
        return generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj, None
    if name == "gen32":
        return generated_long_chain(32, 3232), "l0", "l32", None
    return generated_long_chain(20, 2020), "l0", "l20", (PERMUTED_12 if name == "gen20_permuted" else None)


def _pair(name):
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    xml, base, tool, inputs = _spec(name)
    chain, ref = Chain(xml, base, tool, GRAV), OracleChain(xml, base, tool, GRAV, input_joint_names=inputs)
    if inputs:
        assert chain.setInputJointsName(inputs)
    assert chain.getActiveJointsNumber() == ref.n
    return chain, ref


def _chain(name, gravity=GRAV):
    from rosdyn_amd import Chain
    xml, base, tool, inputs = _spec(name)
    chain = Chain(xml, base, tool, gravity)
    if inputs:
        assert chain.setInputJointsName(inputs)
    return chain


def _cpair(name, oracle=True):
    """(chain, oracle chain or None); ur10_permuted is ur10_like with its input joints permuted"""
    if name != "ur10_permuted":
        return _pair(name) if oracle else (_chain(name), None)
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    f, base, tool = FILES["ur10_like"]
    chain = Chain(os.path.join(FIXTURES, f), base, tool, GRAV)
    names = chain.getActiveJointsName()
    order = [names[i] for i in (4, 0, 5, 2, 1, 3)]
    assert chain.setInputJointsName(order) and chain.getActiveJointsName() == order
    ref = OracleChain(os.path.join(FIXTURES, f), base, tool, GRAV, input_joint_names=order) if oracle else None
    return chain, ref


# planar_2r: the smallest chain; ur10_like, panda_like: 6 and 7 joints; mixed_joints: prismatic joints; ur10_public: fixed head and tail links
# inside a swept chain, the tool a fixed link; ur10_permuted: input order differs from chain order; rev10: the largest register kernel;
# ur10_public_long: a reduced companion without wrenches, the chunked route on the original chain with them; rev14, gen20_permuted: the
# chunked route, permuted
WRENCH_CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_public", "ur10_permuted", "rev10", "ur10_public_long", "rev14",
                 "gen20_permuted"]


def _trio(name, oracle=False):
    """(chain, oracle chain or None, the same chain with zero gravity)"""
    from rosdyn_amd import Chain
    if name == "ur10_permuted":
        chain, ref = _cpair(name, oracle)
        f, base, tool = FILES["ur10_like"]
        xml, inputs = os.path.join(FIXTURES, f), chain.getActiveJointsName()
    else:
        xml, base, tool, inputs = _spec(name)
        chain, ref = _pair(name) if oracle else (_chain(name), None)
    chain0 = Chain(xml, base, tool, (0.0, 0.0, 0.0))
    if inputs:
        assert chain0.setInputJointsName(inputs)
    assert chain0.getActiveJointsName() == chain.getActiveJointsName() and chain0.getLinksName() == chain.getLinksName()
    return chain, ref, chain0


WIDE_GRAV = (0.2, -0.3, -9.7)


def _chain_case(case):
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    inputs = None
    if case.startswith("rev"):
        nj = int(case[3:])
        xml, tool = generated_revolute_chain(nj, 1000 + nj), "l%d" % nj
    else:   # gen20_twelve_permuted: fixed joints and 12 input joints out of chain order
        xml, tool = generated_long_chain(20, 2020), "l20"
        inputs = ["j13", "j0", "j9", "j4", "j16", "j1", "j7", "j19", "j3", "j10", "j6", "j12"]
    chain, ref = Chain(xml, "l0", tool, WIDE_GRAV), OracleChain(xml, "l0", tool, WIDE_GRAV, input_joint_names=inputs)
    if inputs:
        assert chain.setInputJointsName(inputs)
    return chain, ref


def _ur6():
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    path = os.path.join(FIXTURES, "ur10_like.urdf")
    return Chain(path, "base_link", "wrist_3_link", WIDE_GRAV), OracleChain(path, "base_link", "wrist_3_link", WIDE_GRAV)


FACADE_CHAINS = [("ur10_like.urdf", "base_link", "tool0"), ("mixed_joints.urdf", "world", "tip")]
