"""`python -m xna_basecaller_amd basecaller MODEL_DIR READS_DIR ...` == `bonito basecaller ...`, and `... evaluate MODEL_DIR
--directory CTC_DATA` == `bonito evaluate ...` (bonito/__init__.py:10-33); `... segment CTC_DATA` == the reference's
`src/tools/dtw_segmentation.py CTC_DATA`; `... analyze LIB.fasta CALLS.paf -R CALLS.fastq` == the reference's
`src/tools/analyze_paf.py -p`; `... splice DNA_CTC XNA_CTC OUT --ubs XY --prop-ubs P` == the XNA spliced augmentation of
`bonito train -m per_kmer` (bonito/stitch_chunks.py) written out as ctc-data; `... spike CTC OUT -r KMER.model --ubs XY
--prop-ubs P` == the synthetic spiking of `bonito train --spike` (bonito/spike_chunks.py), likewise; `... synth CTC OUT -r
KMER.model --ubs XY --prop-ubs P` == the fully synthetic chunks of `bonito train --spike --fully_synth`, likewise; `... train
TRAINING_DIR --pretrained MODEL_DIR --directory CTC_DATA -F` == `bonito train -F` at its default --num-unfreeze-top 1: the CRF
head fine-tuned with everything below it frozen; with `--num-unfreeze-top K --no-amp`, K in 2 .. 6, the top K - 1 LSTM layers
are trained with it, in float32."""
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

from . import __version__
from .cli import analyze, basecaller, evaluate, segment, spike, splice, synth, train


def main():
    parser = ArgumentParser("bonito", formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("-v", "--version", action="version", version="%(prog)s {}".format(__version__))
    sub = parser.add_subparsers(title="subcommands", description="valid commands", help="additional help",
                                dest="command")
    sub.required = True
    p = sub.add_parser("basecaller", parents=[basecaller.argparser()])
    p.set_defaults(func=basecaller.main)
    p = sub.add_parser("evaluate", parents=[evaluate.argparser()])
    p.set_defaults(func=evaluate.main)
    p = sub.add_parser("segment", parents=[segment.argparser()])
    p.set_defaults(func=segment.main)
    p = sub.add_parser("analyze", parents=[analyze.argparser()])
    p.set_defaults(func=analyze.main)
    p = sub.add_parser("splice", parents=[splice.argparser()])
    p.set_defaults(func=splice.main)
    p = sub.add_parser("spike", parents=[spike.argparser()])
    p.set_defaults(func=spike.main)
    p = sub.add_parser("synth", parents=[synth.argparser()])
    p.set_defaults(func=synth.main)
    p = sub.add_parser("train", parents=[train.argparser()])
    p.set_defaults(func=train.main)
    args = parser.parse_args()
    args.func(args)


if __name__ == "__main__":
    main()
