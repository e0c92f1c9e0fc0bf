/* Empty on purpose: the reference's qdisc code includes this header and uses nothing from it. */
