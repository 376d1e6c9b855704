"""CPU: the model of Stats.run that the GPU tests compare with (tests/stats_model.py), pinned on the golden lists of cnr-2000 and on hand
graphs for every branch, and the known answers of the package's java_double_str."""
import numpy as np
import pytest

import stats_model as SM


@pytest.fixture(scope="module")
def cnr_model(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.uint64); off[1:] = np.cumsum(deg, dtype=np.uint64)
    return SM.model(off, succ)


def test_cnr2000_counters(cnr_model):
    m = cnr_model
    assert (m["nodes"], m["arcs"], m["loops"], m["dangling"], m["terminal"]) == (325557, 3216152, 87442, 78056, 86959)
    assert (m["num_gaps"], m["tot_gap"], m["tot_loc"]) == (3177612, 5239096399, 13431014501)
    assert (m["min_outdegree"], m["min_outdegree_node"], m["max_outdegree"], m["max_outdegree_node"]) == (0, 3, 2716, 46918)
    assert (m["min_indegree"], m["min_indegree_node"]) == (1, 325468)
    # five nodes share the largest indegree: the downward scan keeps the largest of them (argmax would name another)
    assert (m["max_indegree"], m["max_indegree_node"]) == (18235, 205307)
    assert int(np.count_nonzero(m["indegrees"] == 18235)) == 5 and int(np.argmax(m["indegrees"])) != 205307
    assert m["log_delta"][:19] == [128165, 116003, 153431, 199958, 207507, 143273, 129519, 155261, 200779, 203318, 223148, 308730, 373208, 495279, 68102,
                                   6631, 9383, 6217, 798] and not any(m["log_delta"][19:])
    assert len(m["outdegree_distribution"]) == 2717 and list(m["outdegree_distribution"][:3]) == [78056, 38540, 27423]
    assert len(m["indegree_distribution"]) == 18236 and list(m["indegree_distribution"][:3]) == [0, 137407, 71317]


def test_cnr2000_properties_text(cnr_model, W):
    text = SM.properties(cnr_model)
    kv = dict(l.split("=", 1) for l in text.splitlines())
    assert kv["successoravggap"] == "1648.753" and kv["avglocality"] == "4176.113" and kv["successoravglogdelta"] == "4.425"
    assert kv["percdangling"] == "23.9761393550131" and kv["avgoutdegree"] == "9.878921356321626" and kv["avgindegree"] == kv["avgoutdegree"]
    assert kv["successorlogdeltastats"] == "128165,116003,153431,199958,207507,143273,129519,155261,200779,203318,223148,308730,373208,495279,68102,6631,9383,6217,798"
    assert list(kv) == ["nodes", "arcs", "loops", "successoravggap", "avglocality", "minoutdegree", "maxoutdegree", "minoutdegreenode", "maxoutdegreenode", "dangling",
                        "terminal", "percdangling", "avgoutdegree", "successorlogdeltastats", "successoravglogdelta", "minindegree", "maxindegree", "minindegreenode",
                        "maxindegreenode", "avgindegree"]
    # the package formats the same numbers into the same bytes
    m = cnr_model
    gs = W.GraphStats(m["log_delta"], m["outdegree_distribution"], m["indegree_distribution"], **{k: m[k] for k in SM.SCALARS})
    assert gs.properties() == text
    assert gs.properties(buckets=12, scc_sizes=[5, 1, 1, 3, 1]) == SM.properties(m, buckets=12, scc_sizes=[5, 1, 1, 3, 1])


def test_java_double_str(W):
    for x, s in ((100.0, "100.0"), (0.001, "0.001"), (1e-4, "1.0E-4"), (1.2345678e7, "1.2345678E7"), (9999999.0, "9999999.0"), (0.0, "0.0")):
        assert W.java_double_str(x) == s and SM.java_double(x) == s
    for x in (1e7, 0.00099, 123456.789, 1 / 3, 2.5e-9, 6.02e23, 99.5, float("nan")):
        assert W.java_double_str(x) == SM.java_double(x), x
    assert W.java_double_str(1e7) == "1.0E7" and W.java_double_str(float("nan")) == "NaN"


def _m(lists):
    return SM.model(*SM.csr(lists))


def test_hand_graphs():
    m = _m([[0], [0], []])                                                  # d == 1: a loop, a non-loop; an empty list
    assert (m["arcs"], m["loops"], m["dangling"], m["terminal"], m["num_gaps"], m["tot_gap"], m["tot_loc"]) == (2, 1, 1, 2, 0, 0, 1)
    assert m["log_delta"][0] == 1 and list(m["indegrees"]) == [2, 0, 0]
    assert (m["min_outdegree"], m["min_outdegree_node"], m["max_outdegree"], m["max_outdegree_node"]) == (0, 2, 1, 0)
    assert (m["min_indegree"], m["min_indegree_node"], m["max_indegree"], m["max_indegree_node"]) == (0, 2, 2, 0)
    m = _m([[], [], [], [4, 9], [], [], [], [], [], []])                    # d == 2, first successor above the node: (9 - 4) + int2nat(1) = 7
    assert (m["num_gaps"], m["tot_gap"], m["tot_loc"], m["terminal"]) == (2, 7, 7, 9)
    assert m["log_delta"][0] == 1 and m["log_delta"][2] == 1
    m = _m([[], [], [], [], [], [1, 2, 7]])                                 # first successor below the node: int2nat(-4) = 7 (odd)
    assert (m["num_gaps"], m["tot_gap"], m["tot_loc"]) == (3, 6 + 7, 4 + 3 + 2)
    m = _m([[], [], [], []])                                                # all nodes empty: the maxima stay at node 0, the indegree minimum at the last node
    assert (m["arcs"], m["dangling"], m["terminal"]) == (0, 4, 4)
    assert (m["min_outdegree"], m["min_outdegree_node"], m["max_outdegree"], m["max_outdegree_node"]) == (0, 0, 0, 0)
    assert (m["min_indegree"], m["min_indegree_node"], m["max_indegree"], m["max_indegree_node"]) == (0, 3, 0, 0)
    assert list(m["outdegree_distribution"]) == [4] and list(m["indegree_distribution"]) == [4]
    assert "successorlogdeltastats=\nsuccessoravglogdelta=0\n" in SM.properties(m)
    m = _m([[0]])                                                           # one node, one loop
    assert (m["nodes"], m["arcs"], m["loops"], m["dangling"], m["terminal"]) == (1, 1, 1, 0, 1)
    assert list(m["outdegree_distribution"]) == [0, 1] and list(m["indegree_distribution"]) == [0, 1]
    m = _m([])                                                              # no node at all
    assert (m["min_outdegree"], m["min_indegree"]) == (SM.INT64_MAX, SM.INT64_MAX) and list(m["outdegree_distribution"]) == [0]
    assert "percdangling=NaN\n" in SM.properties(m)
