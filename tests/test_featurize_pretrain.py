"""The categorical atom and bond features of GIN (mvml_gat.featurize: pretrain_atom_features,
pretrain_bond_features, smiles_to_pretrain_bigraph; dgllife 0.3.0 PretrainAtomFeaturizer /
PretrainBondFeaturizer restated, parity with dgllife / RDKit unpinned) against answers derived by
hand, and the 74-d path untouched by the fields the parser now keeps."""
import csv
import os

import numpy as np
import pytest

import mvml_gat
from mvml_gat import featurize as fz

HERE = os.path.dirname(os.path.abspath(__file__))
KEGG = os.path.join(HERE, "golden", "kegg_test_split.csv")


def _feats(smiles):
    m = fz.mol_from_smiles(smiles)
    return m, fz.pretrain_atom_features(m), fz.pretrain_bond_features(m)


def test_acetic_acid():
    # C C (=O) O: bonds in creation order 0-1 single, 1-2 double, 1-3 single
    m, a, b = _feats("CC(=O)O")
    assert a["atomic_number"].tolist() == [5, 5, 7, 7] and a["chirality_type"].tolist() == [0, 0, 0, 0]  # Z - 1
    assert b["bond_type"].tolist() == [0, 0, 1, 1, 0, 0, 4, 4, 4, 4]  # both directions of a bond, then 4 self-loops
    assert b["bond_direction_type"].tolist() == [0] * 10
    assert a["atomic_number"].dtype == np.int64 and b["bond_type"].dtype == np.int64
    g = fz.smiles_to_pretrain_bigraph("CC(=O)O")
    assert g.src.tolist() == [0, 1, 1, 2, 1, 3, 0, 1, 2, 3] and g.dst.tolist() == [1, 0, 2, 1, 3, 1, 0, 1, 2, 3]
    assert sorted(g.ndata) == ["atomic_number", "chirality_type"] and sorted(g.edata) == ["bond_direction_type", "bond_type"]
    assert g.edata["bond_type"].tolist() == b["bond_type"].tolist() and g.ndata["atomic_number"].tolist() == [5, 5, 7, 7]
    # without self-loops: the self-loop rows are gone
    nl = fz.smiles_to_pretrain_bigraph("CC(=O)O", add_self_loop=False)
    assert nl.num_edges() == 6 and nl.edata["bond_type"].tolist() == [0, 0, 1, 1, 0, 0]
    assert fz.pretrain_bond_features(m, self_loop=False)["bond_direction_type"].tolist() == [0] * 6


def test_benzene_and_hydrogen_cyanide():
    m, a, b = _feats("c1ccccc1")
    assert a["atomic_number"].tolist() == [5] * 6
    assert b["bond_type"].tolist() == [3] * 12 + [4] * 6  # aromatic; the ring-closure bond 5-0 is the last bond
    assert m.bonds[5][:2] == (0, 5)
    _, _, k = _feats("C1=CC=CC=C1")  # perceived aromatic, as RDKit's sanitisation does
    assert k["bond_type"].tolist() == [3] * 12 + [4] * 6
    _, a, b = _feats("C#N")
    assert a["atomic_number"].tolist() == [5, 6] and b["bond_type"].tolist() == [2, 2, 4, 4]
    _, a, _ = _feats("[Na+].[Cl-]")
    assert a["atomic_number"].tolist() == [10, 16]


def test_double_bond_directions():
    _, _, e = _feats("F/C=C/F")
    _, _, z = _feats("F/C=C\\F")
    assert e["bond_type"].tolist() == z["bond_type"].tolist() == [0, 0, 1, 1, 0, 0, 4, 4, 4, 4]
    assert e["bond_direction_type"].tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 0, 0]  # '/' = 1 on both directions
    assert z["bond_direction_type"].tolist() == [1, 1, 0, 0, 2, 2, 0, 0, 0, 0]  # '\' = 2
    _, _, r = _feats("C/1CC\\1")  # a direction at a ring-closure digit stays with that bond
    assert r["bond_direction_type"].tolist()[:6] == [0, 0, 0, 0, 2, 2]


def test_alanine_enantiomers():
    # written neighbour order of the centre: N, C (methyl), C (carboxyl) = its bonds 0, 1, 2: even
    ml, l, _ = _feats("N[C@@H](C)C(=O)O")
    md, d, _ = _feats("N[C@H](C)C(=O)O")
    assert ml.written[1] == [0, 1, 2] and ml.chiral == [0, 2, 0, 0, 0, 0] and md.chiral == [0, 1, 0, 0, 0, 0]
    assert l["chirality_type"].tolist() == [0, 1, 0, 0, 0, 0]  # '@@': clockwise
    assert d["chirality_type"].tolist() == [0, 2, 0, 0, 0, 0]  # '@': anticlockwise
    assert l["atomic_number"].tolist() == d["atomic_number"].tolist() == [6, 5, 5, 5, 7, 7]


def test_ring_closure_stereocentre_flips_parity():
    # [C@]1(F)(Cl)CCO1: written order ring-1, F, Cl, C; the ring bond is created last (at the closing
    # digit): bonds 5, 0, 1, 2 -> three inversions, odd: '@' (anticlockwise as written) is clockwise
    # in bond order
    m, a, _ = _feats("[C@]1(F)(Cl)CCO1")
    assert m.written[0] == [5, 0, 1, 2] and a["chirality_type"].tolist()[0] == fz.CHI_CW == 1
    _, b, _ = _feats("[C@@]1(F)(Cl)CCO1")
    assert b["chirality_type"].tolist()[0] == fz.CHI_CCW == 2
    # F[C@]1(Cl)CCO1: F, ring-1, Cl, C = bonds 0, 5, 1, 2 -> two inversions, even: no flip
    m, c, _ = _feats("F[C@]1(Cl)CCO1")
    assert m.written[1] == [0, 5, 1, 2] and c["chirality_type"].tolist() == [0, 2, 0, 0, 0, 0]
    # the ring closing AT the centre is created when it is written: C1CCO[C@]1(F)Cl -> bonds 3, 4, 5, 6
    m, d, _ = _feats("C1CCO[C@]1(F)Cl")
    assert m.written[4] == [3, 4, 5, 6] and d["chirality_type"].tolist()[4] == 2
    assert fz._odd_permutation([5, 0, 1, 2]) and not fz._odd_permutation([0, 5, 1, 2]) and not fz._odd_permutation([])


def test_removed_hydrogens_and_canonical_order():
    m, a, b = _feats("[H]C(F)(Cl)Br")  # the explicit H is removed: its bond leaves the lists
    assert m.num_atoms == 4 and a["atomic_number"].tolist() == [5, 8, 16, 34] and len(m.bond_dir) == 3
    assert m.written[0] == [0, 1, 2] and b["bond_type"].tolist() == [0] * 6 + [4] * 4
    plain = fz.smiles_to_pretrain_bigraph("OC(=O)C")
    canon = fz.smiles_to_pretrain_bigraph("OC(=O)C", canonical_atom_order=True)
    assert sorted(canon.ndata["atomic_number"].tolist()) == sorted(plain.ndata["atomic_number"].tolist()) == [5, 5, 7, 7]
    assert canon.edata["bond_type"].tolist() == plain.edata["bond_type"].tolist()  # the bonds keep their order
    z_plain, z_canon = plain.ndata["atomic_number"].tolist(), canon.ndata["atomic_number"].tolist()
    for k in range(3):  # bond k joins the same elements after the renumbering
        assert sorted((z_plain[plain.src[2 * k]], z_plain[plain.dst[2 * k]])) == sorted(
            (z_canon[canon.src[2 * k]], z_canon[canon.dst[2 * k]]))


def test_batch_concatenates_the_edge_features_in_edge_order():
    gs = [fz.smiles_to_pretrain_bigraph(s) for s in ("F/C=C\\F", "C#N", "N[C@H](C)C(=O)O")]
    bg = mvml_gat.batch(gs)
    assert bg.edata["bond_type"].tolist() == sum((g.edata["bond_type"].tolist() for g in gs), [])
    assert bg.edata["bond_direction_type"].tolist() == [1, 1, 0, 0, 2, 2, 0, 0, 0, 0] + [0] * 4 + [0] * 16
    assert bg.ndata["chirality_type"].tolist() == [0] * 4 + [0] * 2 + [0, 2, 0, 0, 0, 0]
    assert bg.num_edges() == 10 + 4 + 16 and bg.edata["bond_type"].shape[0] == bg.num_edges()
    assert max(bg.ndata["atomic_number"].tolist()) < fz.PRETRAIN_NODE_TABLES[0]
    assert max(bg.edata["bond_type"].tolist()) < fz.PRETRAIN_EDGE_TABLES[0]


class _Poison:
    """Stands in for the parser's new fields: any use raises."""

    def __getattr__(self, name):
        raise AssertionError(f"the 74-d path read a stereo field ({name})")

    def __iter__(self):
        raise AssertionError("the 74-d path iterated a stereo field")

    def __getitem__(self, k):
        raise AssertionError("the 74-d path indexed a stereo field")

    def __len__(self):
        raise AssertionError("the 74-d path measured a stereo field")


def _features_without_the_new_fields(smiles):
    """mol_from_smiles + atom_features as before the parser kept the stereo fields: the same steps
    on a molecule whose new fields are poisoned after parsing."""
    m = fz._remove_hs(fz.parse_smiles(smiles))
    m.bond_dir = m.chiral = m.written = _Poison()
    m.implicit_h = [0] * m.num_atoms
    m.implicit_h = [fz._implicit_h(m, i) for i in range(m.num_atoms)]
    assert fz._kekulize(m)
    fz._assign_radicals(m)
    fz._set_aromaticity(m)
    fz._conjugation(m)
    fz._hybridization(m)
    return fz.atom_features(m), [tuple(b) for b in m.bonds]


def test_the_74_features_of_the_kegg_split_do_not_depend_on_the_new_fields():
    with open(KEGG) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 420
    atoms = 0
    for r in rows:
        m = fz.mol_from_smiles(r["smiles"])
        got = fz.atom_features(m)
        want, bonds = _features_without_the_new_fields(r["smiles"])
        assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes(), r["smiles"]
        assert [tuple(b) for b in m.bonds] == bonds
        assert len(m.bond_dir) == len(m.bonds) and len(m.chiral) == len(m.written) == m.num_atoms
        for i in range(m.num_atoms):  # every bond of an atom is in its written order exactly once
            assert sorted(m.written[i]) == sorted(k for (_, k) in m.nbrs(i)), r["smiles"]
        atoms += m.num_atoms
    assert atoms > 5000


@pytest.mark.parametrize("marked,plain", [("F/C=C\\F", "FC=CF"), ("N[C@@H](C)C(=O)O", "N[CH](C)C(=O)O"),
                                          ("[C@]1(F)(Cl)CCO1", "[C]1(F)(Cl)CCO1"), ("C/C=C/c1ccccc1", "CC=Cc1ccccc1")])
def test_stereo_marks_do_not_change_the_74_features(marked, plain):
    a, b = fz.mol_from_smiles(marked), fz.mol_from_smiles(plain)
    assert fz.atom_features(a).tobytes() == fz.atom_features(b).tobytes() and a.bonds == b.bonds
    ga, gb = fz.smiles_to_bigraph(marked), fz.smiles_to_bigraph(plain)
    assert ga.src.tolist() == gb.src.tolist() and ga.ndata["h"].numpy().tobytes() == gb.ndata["h"].numpy().tobytes()
