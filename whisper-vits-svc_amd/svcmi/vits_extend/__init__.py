"""Drop-ins for the pieces of the reference's vits_extend/ that score a checkpoint: stft.TacotronSTFT and stft_loss.MultiResolutionSTFTLoss."""
