"""BondedTable's choice among several matching patterns: the most specific one (fewest wildcards) wins, whatever the order of
the file, as OpenMM prefers a specific match over a wildcard one."""

XML = """<ForceField>
  <AtomTypes>
    <Type name="a" class="A" element="C" mass="12.0"/>
    <Type name="b" class="B" element="C" mass="12.0"/>
  </AtomTypes>
  <PeriodicTorsionForce>
    <Proper type1="" type2="a" type3="b" type4="" periodicity1="2" phase1="3.14" k1="1.0"/>
    <Proper type1="a" type2="a" type3="b" type4="" periodicity1="3" phase1="0.0" k1="2.0"/>
    <Proper class1="A" class2="A" class3="B" class4="B" periodicity1="1" phase1="0.0" k1="3.0" periodicity2="2" phase2="0.5" k2="4.0"/>
  </PeriodicTorsionForce>
  <HarmonicAngleForce>
    <Angle type1="" type2="a" type3="" angle="2.0" k="1.0"/>
    <Angle type1="b" type2="a" type3="b" angle="1.9" k="5.0"/>
  </HarmonicAngleForce>
</ForceField>
"""


def test_the_most_specific_pattern_wins(emdee, tmp_path):
    path = tmp_path / "ff.xml"
    path.write_text(XML)
    t = emdee.ingest.BondedTable(str(path))
    assert t.proper("b", "a", "b", "b") == [(1.0, 2.0, 3.14)]              # only the two-wildcard pattern matches
    assert t.proper("a", "a", "b", "a") == [(2.0, 3.0, 0.0)]               # one wildcard beats two
    assert t.proper("a", "a", "b", "b") == [(3.0, 1.0, 0.0), (4.0, 2.0, 0.5)]   # no wildcard (by class) beats both
    assert t.proper("b", "b", "a", "a") == [(3.0, 1.0, 0.0), (4.0, 2.0, 0.5)]   # ... reversed too
    assert t.angle("b", "a", "b") == [(5.0, 1.9)]
    assert t.angle("a", "a", "b") == [(1.0, 2.0)]
