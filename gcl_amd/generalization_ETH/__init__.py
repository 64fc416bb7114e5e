"""Cross-dataset experiment of the reference (generalization_ETH/): feature-match recall on fragment scenes."""
