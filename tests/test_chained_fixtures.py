"""tests/golden/vorbis/chain_*.ogg.gz and chains.json (written by tests/golden/make_chained_fixtures.py) pin what the chained
Vorbis tests decode: every chain of tests/chained_cases.py, made from its seeds again, must be the committed file byte for byte,
and the models' answer for the committed file -- where its links begin, what each says of itself, the MD5 of each link's PCM -- must be
the recorded one.  And what a player puts out of every link by the granule positions is what the chain was built to hold."""
import os

import pytest

import chained_cases as KC

TABLE = KC.golden_table()


def test_every_chain_has_its_fixture():
    assert sorted(TABLE) == sorted(KC.CHAINS)
    for chain in TABLE:
        assert os.path.getsize(os.path.join(KC.GOLDEN, chain + ".ogg.gz")) < 1 << 20


@pytest.mark.parametrize("chain", sorted(KC.CHAINS))
def test_chain_and_models_are_the_fixtures(chain):
    assert KC.golden(chain) == KC.ogg(chain)
    assert KC.table_entry(chain) == TABLE[chain]
    assert [(r["serial"], r["packets"]) for r in TABLE[chain]["links"]] == [(link[1], link[2] + 3) for link in KC.CHAINS[chain]]


def test_what_a_player_puts_out_of_every_link():
    got = {chain: KC.played(chain) for chain in KC.CHAINS}
    assert [(ch, pcm.shape[0]) for ch, _, pcm in got["chain_mono_stereo"]] == [(1, 1), (2, 2)]
    full = {chain: [r["samples"] for r in TABLE[chain]["links"]] for chain in KC.CHAINS}
    assert [pcm.shape[1] for _, _, pcm in got["chain_million"]] == full["chain_million"]                  # a first granule of 1 000 000 trims nothing
    assert [pcm.shape[1] for _, _, pcm in got["chain_trimmed"]] == [full["chain_trimmed"][0] - 37, full["chain_trimmed"][1]]
    assert [pcm.shape[1] for _, _, pcm in got["chain_negative_g0"]] == [full["chain_negative_g0"][0], full["chain_negative_g0"][1] - 20]
